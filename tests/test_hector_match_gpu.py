"""Directed cases of hs_match_kernel against the CPU oracle, bit for bit (tests/ref/hector_match_cases.py).

tests/test_hector_gpu.py feeds the matcher whole synthetic scans (930 - 1081 points, a good hint).  Here: every
point count up to 400 and the chunk / register-slot boundaries beyond, every instantiation but BIG (SEQ with and
without REGS, the tree order with and without), far hints, points leaving and re-entering the map, the 0.2 rad
clamp at both signs, a singular H, headings across +-pi, a 96 x 80 map with hand-built cells and points placed on the
map limits and on tile / block seams, a point that keeps its cell from one level to the next, and one batched launch over 264 ragged streams (every chain wave).  Both
sides load the same maps (set_map / set_level), so no update kernel takes part in a match-only case.  Compared per
case: the pose bits, the nine covariance bits, the clamp count; the stream's last pose stays untouched and the
Gauss-Newton point counter advances by (6 + 4 (levels - 1)) n.  tests/test_hector_match_cpu.py holds the oracle itself
to the plain float64 statement of the step, and asserts that each case reaches the path it is named after.
"""
import os
import sys

import numpy as np
import pytest

from slam2d.hector import HectorFleet

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "ref"))
import hector_match_cases as K  # noqa: E402

pytestmark = pytest.mark.gpu


def _same_bits(got, want, what):
    """Bit-equal floats; a NaN equals a NaN (the payloads of the host's and the device's NaNs differ)."""
    g = np.ascontiguousarray(got, np.float32).ravel()
    w = np.ascontiguousarray(want, np.float32).ravel()
    ok = (g.view(np.int32) == w.view(np.int32)) | (np.isnan(g) & np.isnan(w))
    assert ok.all(), f"{what}: kernel {g} ({g.view(np.int32)}) oracle {w} ({w.view(np.int32)})"


class Pair:
    """One single-stream fleet and one oracle on the same maps."""

    def __init__(self, geo, edits, max_points, order):
        self.geo = geo
        self.fleet = HectorFleet(1, geo.res, geo.sx, geo.start, geo.levels, max_points=max_points, map_size_y=geo.sy)
        if order:
            self.fleet.set_reduction_order(order)
        self.ora = geo.oracle(reduce_threads=order)
        K.load(self.ora, geo, edits)
        K.load(self.fleet, geo, edits, stream=0)
        self.fleet.counters(reset=True)
        self.state = self.fleet.last_pose(0)
        self.steps = 6 + 4 * (geo.levels - 1)

    def check(self, pts, hint, origo=(0.0, 0.0), what="", counters=True):
        hint = np.asarray(hint, np.float32)
        gp, gc = self.fleet.match(0, pts, hint, origo)
        op, oc = self.ora.match(pts, hint, origo)
        _same_bits(gp, op, f"{what} pose")
        _same_bits(gc, oc, f"{what} covariance")
        assert self.fleet.clamp_count(0) == self.ora.clamp_count(), f"{what} clamp count"
        if counters:
            self.untouched(what, self.steps * int(np.asarray(pts).reshape(-1, 2).shape[0]))
        return gp

    def untouched(self, what, gn_points):
        """A match-only call leaves the stream's pose and covariance alone and counts its points."""
        p, c = self.fleet.last_pose(0)
        _same_bits(p, self.state[0], f"{what} last pose")
        _same_bits(c, self.state[1], f"{what} last covariance")
        assert self.fleet.counters(reset=True)["gn_points"] == gn_points, f"{what} gn_points"

    def close(self):
        self.fleet.close()
        self.ora.close()


@pytest.fixture(scope="module")
def pairs(gpu):
    made = {}

    def get(geo, edits=False, max_points=1152, order=0):
        key = (geo, edits, max_points, order)
        if key not in made:
            made[key] = Pair(*key)
        return made[key]

    yield get
    for p in made.values():
        p.close()


def test_point_counts_seq_regs(pairs):
    """max_points = 1152 (SEQ, REGS: gn_step_cw): every n from 1 to 400 -- every chunk tail of the chain wave's
    unrolled sum, every wave straddling n -- and the chunk and slot boundaries up to 1152."""
    pair = pairs(K.G256)
    before = pair.ora.clamp_count()
    total = 0
    for n in K.COUNTS_1152:
        hint = (0.02, -0.01, 0.01) if n % 2 else (0.33, 0.03, 0.08)
        pair.check(K.scan(K.G256.res, n), hint, what=f"n = {n}", counters=False)
        total += pair.steps * n
    pair.untouched("sweep", total)
    assert pair.ora.clamp_count() >= before


@pytest.mark.parametrize("max_points,order,counts", K.OTHER_INSTANCES, ids=lambda v: str(v) if isinstance(v, int) else "n")
def test_other_instantiations(pairs, max_points, order, counts):
    """SEQ without REGS (max_points 1153 and 2000: gn_step_cw up to 1152 points, the HBM gn_step beyond, with its
    split gathers), the tree order with REGS (1280) and without (1281, 1537): against the oracle in the same order."""
    pair = pairs(K.G256.with_levels(3), max_points=max_points, order=order)
    for n in counts:
        for hint in ((0.02, -0.01, 0.01), (0.3, 0.2, 0.3)):
            pair.check(K.scan(K.G256.res, n), hint, what=f"max_points {max_points} order {order} n = {n} hint {hint}")


@pytest.mark.parametrize("levels", [1, 2, 3, 4])
def test_hints(pairs, levels):
    """Exact, near and far hints, a pure rotation, points leaving the map and returning, every point off the map
    (the pose is the hint, bit for bit), headings at and beyond +-pi, NaN hints: 300 and 1000 points."""
    pair = pairs(K.G256.with_levels(levels))
    cases = [c for c in K.hint_cases() if c.geo.levels == levels]
    assert len(cases) == 28
    for c in cases:
        gp = pair.check(c.pts, c.hint, c.origo, what=c.name)
        if c.expect == "all_out":
            _same_bits(gp, np.asarray(c.hint, np.float32), f"{c.name}: the hint comes back")
        if c.expect == "nan":
            assert np.isnan(gp).any(), c.name


def test_singular_hessian_and_clamps(pairs):
    """A singular H with a non-zero diagonal (the pose turns NaN in mid-match, the same NaNs, the stream's state
    untouched), runaway matches cut at 0.2 rad, and the two directed clamp cases (+0.2 and -0.2)."""
    for c in K.nan_cases() + K.clamp_cases():
        pair = pairs(c.geo, c.edits)
        before = pair.ora.clamp_count()
        gp = pair.check(c.pts, c.hint, c.origo, what=c.name)
        if c.expect == "nan_mid":
            assert np.isnan(gp).all(), gp
        else:
            assert pair.fleet.clamp_count(0) > before and np.isfinite(gp).all(), c.name


# the instances the geometry cases run through: (max_points, order, points added to reach the HBM-strided path)
GEO_INSTANCES = [(1152, 0, 0), (1280, 256, 0), (1800, 0, 1200), (1800, 256, 1290)]


@pytest.mark.parametrize("max_points,order,pad", GEO_INSTANCES)
def test_geometry(pairs, max_points, order, pad):
    """The 96 x 80 map (3 levels: 48 x 40, 24 x 20; padded tiles), map_start (0.01, 0.5), origo != 0, hand-built cells
    (0, +-50, 50 + lo, -200, 80), points exactly on x = 0, on x = sx - 2 and y = sy - 2 (inside), one ulp beyond
    (outside), on both sides of the tile seam (64, 32) and of 4-cell block seams: through gn_step_cw, the tree
    order's gn_step_reg and, padded past the register slots, both orders' HBM-strided gn_step."""
    for c in K.geometry_cases():
        pair = pairs(c.geo, c.edits, max_points, order)
        pts = np.concatenate([c.pts, K.scan(c.geo.res, pad)]) if pad else c.pts
        assert pts.shape[0] <= max_points and (not pad or pts.shape[0] > (1280 if order else 1152))
        pair.check(pts, c.hint, c.origo, what=f"{c.name} max_points {max_points} order {order}")


@pytest.mark.parametrize("max_points,order", [(1152, 0), (1280, 256)])
def test_same_cell_on_two_levels(pairs, max_points, order):
    """A point in cell (0, 0) at the end of one level and at the start of the next: equal cache keys, different
    cells -- the neighbourhood cache (the keys in registers, or nb_key) must be forgotten between levels."""
    for c in K.same_cell_cases():
        pairs(c.geo, c.edits, max_points, order).check(c.pts, c.hint, c.origo, what=f"{c.name} order {order}")


def _torch_dev(a):
    import torch

    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def test_batched_ragged_every_chain_wave(gpu):
    """One launch over 264 streams on equal 128^2 maps, every stream with its own count and hint: the workgroups'
    chain waves take all four values, block ids above 255 add the b >> 8 term.  hs_step_batch_device is the only
    batched entry point, so the first step draws its scan into the map on both sides (a stream's first scan
    always is, unless its pose came out NaN); then the thresholds keep the update away and the second step is a pure
    match.  Some of the few-point streams run away, are cut at 0.2 rad or turn NaN: they are compared like the rest."""
    import torch

    counts, pts, hints = K.batch_cases()
    B = counts.shape[1]
    assert B >= 260 and {(b + (b >> 8)) & 3 for b in range(B)} == {0, 1, 2, 3}
    geo = K.G128
    fleet = HectorFleet(B, geo.res, geo.sx, geo.start, geo.levels, max_points=1152, map_size_y=geo.sy)
    fleet.set_update_factors(0.4, 0.9)
    oras = []
    for s in range(B):
        K.load(fleet, geo, stream=s)
        o = geo.oracle()
        o.set_update_factors(0.4, 0.9)
        K.load(o, geo)
        oras.append(o)
    fleet.counters(reset=True)
    pure = 0
    for t in range(2):
        if t == 1:
            fleet.set_thresholds(1.0e9, 1.0e9)
            for o in oras:
                o.set_thresholds(1.0e9, 1.0e9)
        d_xy, d_n, d_h = _torch_dev(pts[t]), _torch_dev(counts[t]), _torch_dev(hints[t])
        fleet.step_device(d_xy.data_ptr(), 1152, d_n.data_ptr(), 0, d_h.data_ptr())
        torch.cuda.synchronize()
        gp, gc, gd, _ = fleet.poses()
        for s in range(B):
            op, oc, od = oras[s].process(pts[t, s, : counts[t, s]], hint=hints[t, s])
            assert bool(gd[s]) == od, (t, s, od, gd[s])
            pure += t == 1 and not od
            _same_bits(gp[s], op, f"step {t} stream {s} (n = {counts[t, s]}) pose")
            _same_bits(gc[s], oc, f"step {t} stream {s} (n = {counts[t, s]}) covariance")
            assert fleet.clamp_count(s) == oras[s].clamp_count(), (t, s)
    assert pure >= B - 4, pure
    assert fleet.counters()["gn_points"] == 10 * int(counts.sum())
    for s in (0, 1, 61, 131, 164, 204, 241, 256, B - 1):
        for lvl in range(geo.levels):
            m = fleet.get_map(s, lvl)
            ol, ou = oras[s].level(lvl)
            np.testing.assert_array_equal(m["upd"], ou, err_msg=f"stream {s} level {lvl}")
            np.testing.assert_array_equal(m["logodds"].view(np.int32), ol.view(np.int32), err_msg=f"stream {s} level {lvl}")
    fleet.close()
    for o in oras:
        o.close()
