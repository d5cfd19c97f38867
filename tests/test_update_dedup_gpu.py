"""hs_update_kernel rasters each distinct ray once: beams whose end cell equals their predecessor's are dropped in
the ray setup and the survivors packed into consecutive fan groups (csrc/hector_kernels.hip, "Ray setup").

Hand-built point lists whose duplicate structure is known, on 256^2 maps at 1, 2 and 3 levels, against
O.HectorOracle bit for bit: every cell's log-odds and updateIndex, did_update, and the counters cells (the
Bresenham cell count over EVERY valid beam, dropped ones included), rays and touched (distinct cells changed).

Points are in map scale (cells of level 0); with the pose (0, 0, 0) and the map start (0.5, 0.5) a point with
integer coordinates (px, py) ends in cell (128 + px, 128 + py) of level 0, so distinct integer points are distinct
rays there and the number of runs of equal points is level 0's survivor count.  The coarse levels (points scaled by
1/2 and 1/4) merge further neighbours, so their survivor counts differ from level 0's -- more shapes for free.
"""
import numpy as np
import pytest

import oracle as O
from slam2d.hector import HectorFleet

pytestmark = pytest.mark.gpu

SIZE = 256
NAN, INF = float("nan"), float("inf")


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.int32)


def _ring(k, half=100):
    """k distinct integer points in beam order along the square |x|, |y| = half (8 * half cells)."""
    assert k <= 8 * half
    t = (np.arange(k) * (8 * half)) // max(k, 1)  # distinct perimeter positions
    side, o = t // (2 * half), t % (2 * half) - half
    x = np.select([side == 0, side == 1, side == 2], [half, -o, -half], o)
    y = np.select([side == 0, side == 1, side == 2], [o, half, -o], -half)
    p = np.stack([x, y], 1).astype(np.float32)
    assert len({(a, b) for a, b in p.tolist()}) == k
    return p


def _runs(points, lengths):
    """Every point repeated by its run length: a scan with len(points) distinct neighbouring rays at level 0."""
    return np.repeat(np.asarray(points, np.float32).reshape(-1, 2), np.asarray(lengths), axis=0)


def _survivors(k):
    """A scan with exactly k level-0 survivors: k distinct points in runs of 1..3, then beams that draw nothing."""
    # begin == end, NaN, inf, out of map, begin == end again
    junk = np.asarray([(0.0, 0.0), (NAN, 1.0), (INF, 0.0), (1000.0, 3.0), (0.2, -0.3)], np.float32)
    if k == 0:
        return junk
    return np.concatenate([_runs(_ring(k), 1 + np.arange(k) % 3), junk])


def _straddle():
    """300 distinct rays; runs of duplicates across the beams 64 (58..69) and 256 (250..262) of the scan."""
    lengths = np.ones(300, int)
    lengths[58] = 12   # beams 58..69
    # after that run, distinct point j sits at beam j + 11: the run of point 239 covers beams 250..262
    lengths[239] = 13
    return _runs(_ring(300), lengths)


CASES = {
    # every beam on one end cell: one survivor, 299 dropped
    "one_cell": _runs([(60.0, 20.0)], [300]),
    "straddle_64_256": _straddle(),
    "survivors_0": _survivors(0),
    "survivors_1": _survivors(1),
    "survivors_64": _survivors(64),
    "survivors_65": _survivors(65),
    "survivors_256": _survivors(256),
    "survivors_257": _survivors(257),
    # the run's end cell (40, 0) is freed by the EARLIER beam to (80, 0): ((l + lf) - lf) + lo
    "freed_by_earlier": _runs([(80.0, 0.0), (40.0, 0.0), (0.0, 70.0)], [1, 4, 2]),
    # ... and by a LATER beam: the hit comes first, the cell is occupied only
    "freed_by_later": _runs([(0.0, 70.0), (40.0, 0.0), (80.0, 0.0)], [2, 4, 3]),
    # duplicates split by beams that draw nothing: the beam after each is kept again (its predecessor differs)
    "split_by_invalid": np.asarray([(50, 10), (50, 10), (NAN, NAN), (50, 10), (INF, 0), (50, 10), (1000, 0), (50, 10),
                                    (50, 10), (0, 0), (50, 10), (-70, 33), (NAN, 2), (-70, 33)], np.float32),
    # A B A B A: not neighbours, every beam kept
    "a_b_a": _runs([(50.0, 10.0), (50.0, 40.0), (50.0, 10.0), (50.0, 40.0), (50.0, 10.0)], [1, 1, 1, 2, 1]),
}


def _pair(levels, max_points, streams=1):
    fleet = HectorFleet(streams, 0.05, SIZE, (0.5, 0.5), levels, max_points=max_points)
    oras = [O.HectorOracle(0.05, SIZE, (0.5, 0.5), levels, reduce_threads=0) for _ in range(streams)]
    for f in [fleet] + oras:
        f.set_update_factors(0.4, 0.9)
        f.set_thresholds(-1.0, -1.0)
    return fleet, oras


def _same_levels(fleet, ora, levels, what, stream=0):
    for lvl in range(levels):
        m = fleet.get_map(stream, lvl)
        ol, ou = ora.level(lvl)
        np.testing.assert_array_equal(m["upd"], ou, err_msg=f"{what} level {lvl} updateIndex")
        np.testing.assert_array_equal(_bits(m["logodds"]), _bits(ol), err_msg=f"{what} level {lvl} log-odds")
        assert m["update_index"] == ora.update_index(lvl), (what, lvl)


def _touched_since(ora, levels, base):
    """Cells the oracle's last update changed: their updateIndex is one of its two marks (base[lvl] + 1, + 2)."""
    return sum(int((ora.level(lvl)[1] > base[lvl]).sum()) for lvl in range(levels))


def _update_only(levels, pts, max_points, poses):
    """matchData on the empty maps (stores the container the coarse levels draw, moves nothing), then one
    updateByScan (MODE_UPDATE_ONLY) per pose: maps and counters after every update."""
    fleet, (ora,) = _pair(levels, max_points)
    hint = np.zeros(3, np.float32)
    fleet.match(0, pts, hint)  # (its pose is not the subject here: a scan with NaN points has none)
    ora.match(pts, hint)
    want = {"cells": 0, "rays": 0, "touched": 0}
    for k, pose in enumerate(poses):
        pose = np.asarray(pose, np.float32)
        base = [ora.cur_update_index(lvl) for lvl in range(levels)]
        fleet.update_by_scan(0, pts, pose)
        ora.update_by_scan(pts, pose)
        want["cells"] += ora.sum_L()
        want["rays"] += ora.valid_rays()
        want["touched"] += _touched_since(ora, levels, base)
        _same_levels(fleet, ora, levels, f"update {k}")
        got = fleet.counters(reset=False)
        assert {n: got[n] for n in want} == want, (k, got, want)
    return want


# the same scan twice from (0, 0, 0) (the second update meets its own marks' values: hit cells near and past the
# clamp, freed cells again), then from a shifted, rotated pose (other duplicates, the old cells stay)
POSES = [(0.0, 0.0, 0.0), (0.0, 0.0, 0.0), (0.35, -0.2, 0.4)]


@pytest.mark.parametrize("levels", [1, 2, 3])
@pytest.mark.parametrize("case", sorted(CASES))
def test_hand_built_duplicates(gpu, case, levels):
    pts = CASES[case]
    want = _update_only(levels, pts, max(len(pts), 16), POSES)
    if case == "survivors_0":
        assert want == {"cells": 0, "rays": 0, "touched": 0}
    else:
        assert want["rays"] > 0 and want["touched"] > 0


@pytest.mark.parametrize("levels", [1, 2, 3])
def test_rays_in_lds_instance(gpu, levels):
    """About 1400 points (more than the 1280 the register instance holds: hs_update_kernel<0>, rays packed inside
    their LDS array): 350 distinct rays in runs of 4, so every thread's chunk of 6 beams straddles runs."""
    pts = _runs(_ring(350), np.full(350, 4))
    assert len(pts) == 1400
    _update_only(levels, pts, 1400, POSES)


@pytest.mark.parametrize("levels", [1, 2, 3])
def test_three_steps_with_ordinal_sweep(gpu, monkeypatch, levels):
    """Two streams with different (ragged) duplicate scans through hs_step_batch_device -- match, gate (forced),
    update -- for three consecutive steps with an ordinal sweep before each: poses, did_update, maps, counters."""
    import torch

    monkeypatch.setenv("SLAM2D_ORD_SWEEP", "1")
    scans = [CASES["straddle_64_256"], _runs(_ring(90, half=60), 1 + np.arange(90) % 5)]
    stride = max(len(p) for p in scans)
    fleet, oras = _pair(levels, stride, streams=2)
    xy = np.zeros((2, stride, 2), np.float32)
    for s, p in enumerate(scans):
        xy[s, : len(p)] = p
    d_xy = torch.from_numpy(xy).cuda()
    d_n = torch.tensor([len(p) for p in scans], dtype=torch.int32).cuda()
    want = {"cells": 0, "rays": 0, "touched": 0}
    for t in range(3):
        base = [[o.cur_update_index(lvl) for lvl in range(levels)] for o in oras]
        fleet.step_device(d_xy.data_ptr(), stride, d_n.data_ptr())
        torch.cuda.synchronize()
        gp, _, gd, _ = fleet.poses()
        for s, o in enumerate(oras):
            op, _, od = o.process(scans[s])
            assert bool(gd[s]) == od, (t, s)
            np.testing.assert_array_equal(_bits(gp[s]), _bits(op), err_msg=f"step {t} stream {s} pose")
            want["cells"] += o.sum_L()
            want["rays"] += o.valid_rays()
            want["touched"] += _touched_since(o, levels, base[s])
            _same_levels(fleet, o, levels, f"step {t} stream {s}", stream=s)
        got = fleet.counters(reset=False)
        assert {n: got[n] for n in want} == want, (t, got, want)
