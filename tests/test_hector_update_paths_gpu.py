"""The Hector grid-update kernels against the oracle on directed inputs, through every launch path.

Cases and paths: tests/ref/hector_update_cases.py (the table is in DESIGN.md section 3).  tests/test_hector_update_cpu.py
holds the oracle to the plain statement on the same cases and asserts that each case reaches what it claims; here
hs_update_kernel<5> (rays in registers), hs_update_kernel<0> (rays in LDS), hs_update_ring_kernel and hs_bin_kernel +
hs_tile_kernel meet that oracle.  After every update, bit for bit: every cell's log-odds (as int32, NaN payloads
included), every cell's decoded updateIndex, update_index, the occ publish bytes, and the counters cells, rays and
touched; queue_stats()["items"] tells the single kernels (0) from the binned ones.

The oracle's maps of a case are computed once and shared by the paths that run it (the tests are ordered by case).
"""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "ref"))
import hector_update_cases as K  # noqa: E402
from slam2d.hector import HectorFleet  # noqa: E402

pytestmark = pytest.mark.gpu

PLAN = sorted(K.plan(), key=lambda pc: (pc[1], pc[0]))
_ORACLE = {}   # the last case's oracle snapshots (one entry: a limit case's maps are some 10 MB per update)


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.int32)


def _snapshot(ora, levels):
    return [(_bits(ora.level(lvl)[0]).copy(), ora.level(lvl)[1].copy(), ora.update_index(lvl), ora.publish(lvl).copy())
            for lvl in range(levels)]


def oracle_run(case):
    """[(per-level snapshot, counters)] after every update of the case, from O.HectorOracle."""
    if case.name not in _ORACLE:
        _ORACLE.clear()
        geo = case.geo
        ora = K.make_oracle(geo)
        init = K.init_levels(case)
        out = []
        for k, u in enumerate(case.updates):
            if geo.levels > 1:
                ora.match(u.pts, u.pose, u.origo)
            if k == 0 and init:
                for lvl, (l, ui) in enumerate(init):
                    ora.set_level(lvl, l, ui)
            base = [ora.cur_update_index(lvl) for lvl in range(geo.levels)]
            ora.update_by_scan(u.pts, u.pose, u.origo)
            out.append((_snapshot(ora, geo.levels),
                        dict(cells=ora.sum_L(), rays=ora.valid_rays(), touched=K.touched_since(ora, geo.levels, base))))
        _ORACLE[case.name] = out
    return _ORACLE[case.name]


def _same(fleet, snap, what, stream=0):
    for lvl, (l_bits, upd, ui, occ) in enumerate(snap):
        m = fleet.get_map(stream, lvl)
        np.testing.assert_array_equal(_bits(m["logodds"]), l_bits, err_msg=f"{what} level {lvl} log-odds")
        np.testing.assert_array_equal(m["upd"], upd, err_msg=f"{what} level {lvl} updateIndex")
        assert m["update_index"] == ui, (what, lvl)
        np.testing.assert_array_equal(m["occ"], occ, err_msg=f"{what} level {lvl} occ")


def _fleet(geo, max_points, streams=1, thresholds=(-1.0, -1.0)):
    fleet = HectorFleet(streams, K.RES, geo.sx, geo.start, geo.levels, max_points=max_points, map_size_y=geo.sy)
    fleet.set_update_factors(K.FREE, K.OCC)
    fleet.set_thresholds(*thresholds)
    return fleet


def run_case(monkeypatch, path, case, extra_env=()):
    assert path.admits(case)
    for k, v in tuple(path.env) + tuple(case.env.items()) + tuple(extra_env):
        monkeypatch.setenv(k, v)
    geo = case.geo
    want_all = oracle_run(case)
    fleet = _fleet(geo, path.max_points(case))
    init = K.init_levels(case)
    want = dict(cells=0, rays=0, touched=0)
    for k, u in enumerate(case.updates):
        if geo.levels > 1:   # matchData stores the container the coarse levels draw
            fleet.match(0, u.pts, u.pose, u.origo)
        if k == 0 and init:
            for lvl, (l, ui) in enumerate(init):
                fleet.set_map(0, lvl, l, ui)
        fleet.update_by_scan(0, u.pts, u.pose, u.origo)
        snap, cnt = want_all[k]
        for n in want:
            want[n] += cnt[n]
        _same(fleet, snap, f"{path.name} {case.name} update {k}")
        got = fleet.counters(reset=False)
        assert {n: got[n] for n in want} == want, (path.name, case.name, k, got, want)
        q = fleet.queue_stats()
        if path.kernel == "binned":
            assert (q["items"] + q["whole"] > 0) == (cnt["rays"] > 0), (case.name, k, q)
        else:
            assert q["items"] == 0 and q["whole"] == 0, (case.name, k, q)
    return fleet, want


@pytest.mark.parametrize("pname,cname", PLAN, ids=[f"{p}-{c}" for p, c in PLAN])
def test_update_paths(gpu, monkeypatch, pname, cname):
    case = K.all_cases()[cname]
    fleet, want = run_case(monkeypatch, K.PATHS[pname], case)
    if case.kind == "limit":
        assert want["cells"] > sum(case.da_sum)
    if case.kind == "g7":
        q = fleet.queue_stats()
        if case.geo is K.G7:   # a box of 33 x 33 tiles: the MAX_BIN_TILES fallback, one WHOLE item
            assert q["whole"] > 0 and q["overflow"] == 0, q
        else:                  # 32 x 32 = MAX_BIN_TILES tiles: still one item per non-empty tile
            assert q["whole"] == 0 and q["overflow"] == 0 and q["items"] > 32, q


def test_binned_item_overflow(gpu, monkeypatch):
    """G4's every_cell with room for 8 tile items: the queue overflows and the levels fall back to WHOLE items."""
    case = K.all_cases()["every_G4_48_40"]
    fleet, _ = run_case(monkeypatch, K.PATHS["binned"], case, extra_env=(("SLAM2D_ITEM_CAP", "8"),))
    q = fleet.queue_stats()
    assert q["overflow"] > 0, q


@pytest.mark.parametrize("pname", ["regs", "parts321", "split532"])
def test_batch(gpu, monkeypatch, pname):
    """One step_device launch over 6 ragged streams (two of them empty), each another case's scan, on G4's map: per-stream
    hints make some streams pass the update gate (0.4, 0.9) and others not, for 3 steps -- poses, did_update, maps and
    counters.  (regs: the list-driven split -- the instance is the LDS one, the longest scan has 7679 points.)"""
    import torch

    for k, v in K.PATHS[pname].env:
        monkeypatch.setenv(k, v)
    scans, hints = K.batch_scans()
    stride = max(len(p) for p in scans)
    fleet = _fleet(K.G4, stride, streams=len(scans), thresholds=(0.4, 0.9))
    oras = [K.make_oracle(K.G4) for _ in scans]
    for o in oras:
        o.set_thresholds(0.4, 0.9)
    xy = np.zeros((len(scans), stride, 2), np.float32)
    for s, p in enumerate(scans):
        xy[s, : len(p)] = p
    d_xy = torch.from_numpy(xy).cuda()
    d_n = torch.tensor([len(p) for p in scans], dtype=torch.int32).cuda()
    want = dict(cells=0, rays=0, touched=0)
    mixed = 0
    for t in range(3):
        d_hints = torch.from_numpy(hints[t].copy()).cuda()
        base = [[o.cur_update_index(lvl) for lvl in range(3)] for o in oras]
        fleet.step_device(d_xy.data_ptr(), stride, d_n.data_ptr(), d_hints=d_hints.data_ptr())
        torch.cuda.synchronize()
        gp, _, gd, _ = fleet.poses()
        dids = []
        for s, o in enumerate(oras):
            op, _, od = o.process(scans[s], hint=hints[t, s])
            dids.append(od)
            assert bool(gd[s]) == od, (t, s)
            np.testing.assert_array_equal(_bits(gp[s]), _bits(op), err_msg=f"step {t} stream {s} pose")
            if od:
                want["cells"] += o.sum_L()
                want["rays"] += o.valid_rays()
                want["touched"] += K.touched_since(o, 3, base[s])
            _same(fleet, _snapshot(o, 3), f"step {t} stream {s}", stream=s)
        mixed += len(set(dids)) == 2
        got = fleet.counters(reset=False)
        assert {n: got[n] for n in want} == want, (t, got, want)
    assert mixed >= 1
