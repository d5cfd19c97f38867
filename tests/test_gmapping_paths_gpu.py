"""Every path of the GMapping particle-map kernels (gm_score_kernel, gm_compute_kernel, gm_publish_kernel) and of their
C-ABI against the GMapping oracle, bit for bit: n, visits, the float accumulators as int32 bits, publish, the hit and
free counts, and the score against the previous oracle map.  No tolerance: integers and float sums in a fixed order
are exact by design.

tests/test_gmapping_gpu.py runs scans of a synthetic world at the default geometry with SLAM2D_GM_PARTS = 5 on all
particles.  Here: directed beams (tests/ref/gmapping_cases.py: every case knows its end cells, and
tests/test_gmapping_cpu.py proves from the oracle alone that they are the oracle's) in every octant, lines of 4000
cells, an off-centre map of 2 x 2 tiles with a 32-cell last column, cells hit by several beams of different waves,
hit cells at one LDS word in consecutive tiles, every special range value, n below the beam cache, 1 / 5 / 16
workgroups per particle, partial launches, reset, the occupancy threshold and the argument errors.
"""
import os
import sys

import numpy as np
import pytest

import oracle as O
from slam2d._lib import Slam2dError
from slam2d.gmapping import GMappingFleet

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "ref"))
import gmapping_cases as G  # noqa: E402

pytestmark = pytest.mark.gpu

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def _fleet(c, P, max_beams=None):
    f = GMappingFleet(P, max_beams=max_beams or len(c.a_cos), **c.p)
    assert f.size == G.dims(c.p)[:2]
    f.set_beams(a_cos=c.a_cos, a_sin=c.a_sin)
    return f


def _check_particle(fleet, k, ref, thresh=0.25, what=""):
    """Particle k's map, publish, hit and free counts == the oracle's (n, visits, acc, nfree, nhits)."""
    on, ov, oacc, nfree, nhits = ref
    n, v, acc = fleet.particle_map(k)
    np.testing.assert_array_equal(v, ov, err_msg=f"{what} particle {k} visits")
    np.testing.assert_array_equal(n, on, err_msg=f"{what} particle {k} n")
    np.testing.assert_array_equal(acc.view(np.int32), oacc.view(np.int32), err_msg=f"{what} particle {k} acc")
    np.testing.assert_array_equal(fleet.publish(k), G.publish(on, ov, thresh), err_msg=f"{what} particle {k} publish")
    _, h, f = fleet.scores()
    assert (h[k], f[k]) == (nhits, nfree), (what, k)


def _run_steps(fleet, c, steps=None, prev=None, thresh=0.25):
    """compute() every step of the case; maps, counts and scores checked after each.  Returns the last maps."""
    maps = G.oracle_maps(c.name)
    P = fleet.P
    prev = prev or [None] * P
    for s in (range(len(c.steps)) if steps is None else steps):
        st = c.steps[s]
        fleet.compute(st.poses4, st.ranges)
        score = fleet.scores()[0]
        for k in range(P):
            _check_particle(fleet, k, maps[s][k], thresh, f"{c.name} step {s}")
            want = G.expected_score(prev[k], st.poses4[k], st.ranges, c.a_cos, c.a_sin, c.p, thresh)
            assert score[k] == want, (c.name, s, k)
            prev[k] = maps[s][k][:2]
    return prev


@pytest.mark.parametrize("parts", [1, 5, 16])
@pytest.mark.parametrize("name", G.FAMILY_CASES)
def test_family_at_parts(gpu, monkeypatch, name, parts):
    """Every case family with 1, 5 and 16 workgroups per particle (SLAM2D_GM_PARTS, read by gm_create).  With one,
    a single workgroup walks every tile of the box in order, so the LDS state it carries from tile to tile (first-hit
    words restored by the acc pass, counts zeroed by the store pass, the two parities of the tile flags) is exercised
    in the order the tile_seq_* and tile_alternating cases arrange; with sixteen, most workgroups of the small cases
    have no tile (one_tile: fifteen of sixteen)."""
    monkeypatch.setenv("SLAM2D_GM_PARTS", str(parts))
    c = G.case(name)
    G.check_intent(name)
    fleet = _fleet(c, len(c.steps[0].poses4))
    try:
        _run_steps(fleet, c)
    finally:
        fleet.close()


@pytest.mark.parametrize("key", [f"{g}{k}" for g in ("small_offset", "fine_long") for k in range(2)])
def test_reference_geometry_fixture(gpu, key):
    """tests/golden/gmapping_ref_geom.npz: the reference build's own sparse outputs at the two other geometries."""
    d = np.load(os.path.join(GOLD, "gmapping_ref_geom.npz"))
    fleet = GMappingFleet(1, max_beams=len(d[f"{key}_a_cos"]), **G.GEOMS[key[:-1]])
    fleet.set_beams(a_cos=d[f"{key}_a_cos"], a_sin=d[f"{key}_a_sin"])
    fleet.compute(d[f"{key}_pose"][None], d[f"{key}_ranges"])
    n, v, acc = fleet.particle_map(0)
    idx = d[f"{key}_idx"]
    np.testing.assert_array_equal(np.nonzero(v.ravel())[0], idx)
    np.testing.assert_array_equal(n.ravel()[idx], d[f"{key}_n"])
    np.testing.assert_array_equal(v.ravel()[idx], d[f"{key}_visits"])
    np.testing.assert_array_equal(acc.reshape(-1, 2)[idx].view(np.int32), d[f"{key}_acc_bits"])
    assert n.sum() == d[f"{key}_n"].sum() and np.count_nonzero(acc.reshape(-1, 2).any(axis=1)) <= len(idx)
    _, h, f = fleet.scores()
    assert [f[0], h[0]] == list(d[f"{key}_counts"])
    fleet.close()


@pytest.mark.parametrize("parts", [1, 5])
def test_stale_tiles_and_score(gpu, monkeypatch, parts):
    """A particle that jumps away and comes back: steps at A, B (a disjoint tile box), A, A.  A's tiles of step 1 are
    still in memory at step 3 but two steps stale: every map equals a fresh oracle map, the score is 0 at steps 2
    and 3 (against the intermediate map) and positive at step 4.  Step 5, two beams to opposite corners of the same
    box, covers tiles written at step 4 that now receive no mark: they read as zero.  (Particle 1: B, A, B, B.)"""
    monkeypatch.setenv("SLAM2D_GM_PARTS", str(parts))
    c = G.case("stale_tiles")
    maps = G.oracle_maps("stale_tiles")
    fleet = _fleet(c, 2)
    prev = [None, None]
    scores = []
    for s in range(5):
        prev = _run_steps(fleet, c, steps=[s], prev=prev)
        scores.append(fleet.scores()[0].copy())
    assert [list(x) for x in scores[:3]] == [[0, 0]] * 3
    assert (scores[3] > 100).all() and (scores[4] >= 0).all()
    # step 5's unmarked tiles held step 4's counts
    for k in range(2):
        gone = (maps[3][k][1] > 0) & (maps[4][k][1] == 0)
        assert gone.sum() > 1000 and (fleet.particle_map(k)[1][gone] == 0).all() and (fleet.publish(k)[gone] == -1).all()
    fleet.close()


def test_threshold_boundary(gpu):
    """occ > thresh: a cell at n / visits == 0.25 exactly is not occupied at the default threshold.  Step 1 leaves X at
    n = 1, visits = 4 and Y at n = 2, visits = 4; step 2's one hit beam lands on X for particle 0 and on Y for
    particle 1.  gm_set_occ_thresh moves both the score and publish; publish before any step is all -1."""
    c = G.case("threshold")
    maps = G.oracle_maps("threshold")
    (xx, xy), (yx, yy) = G.THRESH_X, G.THRESH_Y
    fleet = _fleet(c, 2)
    assert (fleet.publish(0) == -1).all() and (fleet.publish(1) == -1).all()
    for thresh, want_score, want_pub in ((None, [0, 1], (0, 100)), (0.2, [1, 1], (100, 100)), (0.5, [0, 0], (0, 0)),
                                         (0.25, [0, 1], (0, 100))):
        if thresh is not None:
            fleet.reset()
            fleet.set_occ_thresh(thresh)
        t = 0.25 if thresh is None else thresh
        _run_steps(fleet, c, steps=[0], thresh=t)
        pub = fleet.publish(0)
        assert (pub[xy, xx], pub[yy, yx]) == want_pub, thresh
        _run_steps(fleet, c, steps=[1], prev=[m[:2] for m in maps[0]], thresh=t)
        assert list(fleet.scores()[0]) == want_score, thresh
    fleet.close()


def test_partial_launches(gpu):
    """gm_compute_maps_device on particles [2, 4) of 5: poses and d_scores_out are indexed by the local block, state
    by begin + block.  Particles 0, 1 and 4 keep their map, score, hits and free counts; 2 and 3 match the oracle; the
    following full launch scores every particle against its own previous map; count = 0 does nothing."""
    import torch

    c = G.case("partial")
    maps = G.oracle_maps("partial")
    P = 5
    fleet = _fleet(c, P)
    hs = torch.cuda.current_stream().cuda_stream
    _run_steps(fleet, c, steps=[0])
    s0, h0, f0 = fleet.scores()
    # the 2-pose array heads a longer buffer whose other entries are a pose nobody uses, and the 2-entry score
    # buffer lies between guard words: an index by the global particle number stays inside both, and shows
    st = c.steps[1]
    decoy = np.asarray(G.cell_pose(c.p, 5, 5), np.float64)
    host_poses = np.concatenate([st.poses4[2:4], np.tile(decoy, (P, 1))])
    d_poses = torch.from_numpy(host_poses).cuda()
    d_scores = torch.full((2 + P,), -7, dtype=torch.int32, device="cuda")
    d_r = torch.from_numpy(st.ranges).cuda()
    fleet.compute_device(d_poses.data_ptr(), d_r.data_ptr(), len(st.ranges), d_scores.data_ptr(), begin=2, count=2,
                         hip_stream=hs)
    torch.cuda.synchronize()
    s1, h1, f1 = fleet.scores()
    want = [G.expected_score(maps[0][k][:2], st.poses4[k], st.ranges, c.a_cos, c.a_sin, c.p) for k in (2, 3)]
    assert want[0] > 0 and want[1] > 0
    assert d_scores.cpu().tolist() == want + [-7] * P
    assert list(s1[2:4]) == want
    for k in (0, 1, 4):
        _check_particle(fleet, k, maps[0][k], what="untouched")
        assert (s1[k], h1[k], f1[k]) == (s0[k], h0[k], f0[k])
    for k in (2, 3):
        _check_particle(fleet, k, maps[1][k], what="partial")
    # count = 0: nothing moves, at any begin
    for begin in (0, 2, P):
        fleet.compute_device(d_poses.data_ptr(), d_r.data_ptr(), len(st.ranges), d_scores.data_ptr(), begin=begin,
                             count=0, hip_stream=hs)
    torch.cuda.synchronize()
    for a, b in zip(fleet.scores(), (s1, h1, f1)):
        np.testing.assert_array_equal(a, b)
    assert d_scores.cpu().tolist() == want + [-7] * P
    _check_particle(fleet, 0, maps[0][0], what="after count = 0")
    _check_particle(fleet, 2, maps[1][2], what="after count = 0")
    # a full launch: each particle against its own previous map (step 1's for 0, 1, 4; step 2's for 2, 3)
    prev = [maps[1][k][:2] if k in (2, 3) else maps[0][k][:2] for k in range(P)]
    want2 = [G.expected_score(prev[k], c.steps[2].poses4[k], c.steps[2].ranges, c.a_cos, c.a_sin, c.p) for k in range(P)]
    other = [G.expected_score(maps[1][k][:2] if k not in (2, 3) else maps[0][k][:2], c.steps[2].poses4[k],
                              c.steps[2].ranges, c.a_cos, c.a_sin, c.p) for k in range(P)]
    assert want2 != other   # the two histories tell apart
    _run_steps(fleet, c, steps=[2], prev=prev)
    assert list(fleet.scores()[0]) == want2
    fleet.close()


def test_reset(gpu):
    """gm_reset after two steps: empty maps, publish all -1, and the next step scores 0 and equals, map and counters,
    that step on a newly created fleet."""
    c = G.case("partial")
    maps = G.oracle_maps("partial")
    P = 5
    fleet = _fleet(c, P)
    _run_steps(fleet, c, steps=[0, 1])
    assert fleet.scores()[0].max() > 0
    fleet.reset()
    for k in range(P):
        n, v, acc = fleet.particle_map(k)
        assert not n.any() and not v.any() and not acc.any()
        assert (fleet.publish(k) == -1).all()
    _run_steps(fleet, c, steps=[2])      # prev = None: every score 0
    assert not fleet.scores()[0].any()
    fresh = _fleet(c, P)
    _run_steps(fresh, c, steps=[2])
    for a, b in zip(fleet.scores(), fresh.scores()):
        np.testing.assert_array_equal(a, b)
    for k in range(P):
        for a, b in zip(fleet.particle_map(k), fresh.particle_map(k)):
            np.testing.assert_array_equal(a.view(np.int32), b.view(np.int32))
        _check_particle(fleet, k, maps[2][k], what="after reset")
    fleet.close()
    fresh.close()


BAD_CREATE = {
    "num_particles = 0": dict(num_particles=0),
    "max_beams = 0": dict(max_beams=0),
    "max_beams = 8193": dict(max_beams=8193),
    "delta = 0": dict(delta=0.0),
    "xmax <= xmin": dict(xmax=10.0),
    "ymax < ymin": dict(ymax=-8.0),
    "a map below 32 cells": dict(xmax=11.5),
    "max_range / delta >= 16384": dict(delta=0.001),
}


@pytest.mark.parametrize("what", list(BAD_CREATE))
def test_create_argument_errors(gpu, what):
    kw = dict(G.GEOMS["small_offset"], num_particles=2, max_beams=100)
    GMappingFleet(kw.pop("num_particles"), **kw).close()     # the arguments are good but for the one changed
    kw = dict(G.GEOMS["small_offset"], num_particles=2, max_beams=100)
    kw.update(BAD_CREATE[what])
    with pytest.raises(Slam2dError, match="gm_create failed with code -1"):
        GMappingFleet(kw.pop("num_particles"), **kw)


def test_call_argument_errors_leave_the_fleet_usable(gpu):
    import torch

    c = G.case("partial")
    P = 5
    fleet = _fleet(c, P, max_beams=len(c.a_cos) + 8)
    st = c.steps[0]
    _run_steps(fleet, c, steps=[0])
    nb = len(c.a_cos)
    d_poses = torch.from_numpy(st.poses4).cuda()
    d_r = torch.from_numpy(np.concatenate([st.ranges, st.ranges])).cuda()
    bad = [
        lambda: fleet.set_beams(a_cos=np.ones(nb + 9), a_sin=np.zeros(nb + 9)),            # n > max_beams
        lambda: fleet.compute(st.poses4, np.ones(nb + 1, np.float32)),                     # n > n_beams
        lambda: fleet.compute_device(d_poses.data_ptr(), d_r.data_ptr(), nb + 1),          # n > n_beams
        lambda: fleet.compute_device(d_poses.data_ptr(), d_r.data_ptr(), nb, begin=4, count=2),
        lambda: fleet.compute_device(d_poses.data_ptr(), d_r.data_ptr(), nb, begin=-1, count=1),
        lambda: fleet.compute_device(d_poses.data_ptr(), d_r.data_ptr(), nb, begin=0, count=-1),
        lambda: fleet.compute_device(0, d_r.data_ptr(), nb),
        lambda: fleet.particle_map(P),
        lambda: fleet.particle_map(-1),
        lambda: fleet.publish(P),
    ]
    for i, call in enumerate(bad):
        with pytest.raises(Slam2dError, match="code -1"):
            call()
        torch.cuda.synchronize()
        # nothing moved: the beam cache, the maps and the counters are step 1's
        assert fleet.n_beams == nb
        _check_particle(fleet, i % P, G.oracle_maps("partial")[0][i % P], what=f"after bad call {i}")
    # and the next steps run as if nothing had happened
    _run_steps(fleet, c, steps=[1, 2], prev=[m[:2] for m in G.oracle_maps("partial")[0]])
    fleet.close()
