"""The Hector oracle's grid update held to the plain statement, and the preconditions of the directed update cases.

oracle/hector_oracle.c's update is what the GPU tests compare bits against (tests/test_hector_update_paths_gpu.py).  Its
cell walk and its cell rules were pinned before (tests/test_oracle_cpu.py); its end-cell arithmetic, its bounds test and
its begin == end skip were not.  Here every case of tests/ref/hector_update_cases.py is replayed through the oracle and
through tests/ref/hector_update_plain.py -- numpy float32 end cells, the pure-Python Bresenham, a dict walk of the cell
rules -- and compared bit for bit after every update: log-odds (as int32, so NaN payloads count), updateIndex, the
update indices, the publish bytes and the counters.

test_case_preconditions asserts, from that replay alone, that every case reaches what it claims: a case that does
not fails here, on the CPU, not silently on the GPU.
"""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "ref"))
import hector_update_cases as K  # noqa: E402
import hector_update_plain as P  # noqa: E402

CASES = sorted(K.all_cases())


@pytest.mark.parametrize("name", CASES)
def test_oracle_equals_plain(name):
    diffs, facts = K.replay(name)
    assert not diffs, diffs
    assert len(facts) == len(K.all_cases()[name].updates)


def _kind(kind):
    return [c for c in K.all_cases().values() if c.kind == kind]


def test_plain_statement_itself():
    """The plain statement on a map small enough to follow by hand: 8 x 4, begin (1, 1), beams to (5, 1), (3, 1), (5, 1)."""
    m = P.PlainMap(1.0, 8, 4, (0.0, 0.0), 1, 0.4, 0.9)
    pts = np.asarray([(4, 0), (2, 0), (4, 0), (np.nan, 0), (0.2, 0.2), (100, 0)], np.float32)
    m.update_by_scan(pts, (1.25, 1.25, 0.0))
    l, u = m.level(0)
    lf, lo = P.prob_to_logodds(0.4), P.prob_to_logodds(0.9)
    assert (m.cells, m.rays, m.touched) == (5 + 3 + 5, 3, 5)
    assert u[1].tolist() == [-1, 1, 1, 2, 1, 2, -1, -1] and (u[[0, 2, 3]] == -1).all()
    np.testing.assert_array_equal(l[1], np.asarray([0, lf, lf, (lf - lf) + lo, lf, lo, 0, 0], np.float32))
    assert m.lv[0].cur == 3 and m.lv[0].last == 0
    assert m.publish(0)[1].tolist() == [-1, 0, 0, 100, 0, 100, -1, -1]


def test_case_preconditions():
    cases = K.all_cases()
    # ---- every_cell: every (dx, dy) of the map, every order; the far-first and near-first orders do what they claim
    for c in _kind("every_cell"):
        facts = K.reach(c)
        g = c.geo
        per_order = len(c.updates) // (2 if c.geo is K.G4 else 5)
        for k0 in range(0, len(c.updates), per_order):
            ends = [e for u in c.updates[k0:k0 + per_order] for e in u.ends]
            assert len(ends) == g.sx * g.sy - 1 == len(set(ends)) and c.updates[k0].begin not in ends, c.name
            assert sum(f[0]["nu"] for f in facts[k0:k0 + per_order]) == g.sx * g.sy - 1
        for f in facts:
            assert f[0]["ntx"] * 64 >= g.sx - 63 and f[0]["quad_hit"] > 0
    c = cases["every_G1_20_15"]   # the five orders, one update each
    f = K.reach(c)
    assert f[3][0]["hit_freed_earlier"] > 1000 and f[3][0]["hit_freed_later"] == 0      # far first
    assert f[4][0]["hit_freed_earlier"] == 0 and f[4][0]["hit_freed_later"] > 1000      # near first
    b = c.updates[0].begin
    d = {(e[0] - b[0], e[1] - b[1]) for e in c.updates[0].ends}
    da_db = {(max(abs(x), abs(y)), min(abs(x), abs(y))) for x, y in d}
    assert {(1, 0), (1, 1), (7, 0), (7, 7), (8, 7), (9, 8), (2, 1)} <= da_db and {(-3, 0), (3, 0), (0, 3), (0, -3)} <= d
    # G4: "every cell" is 7679 beams, more than 4096 distinct rays at level 0 (fan groups past the ballot's 64)
    for c in (x for x in _kind("every_cell") if x.geo is K.G4):
        for f in K.reach(c):
            assert f[0]["nu"] == 7679 and f[0]["ntiles"] == 6
            if c.updates[0].begin == (95, 79):
                # the far corner's coarse begin cells, (int)(47.625 + 0.5) = 48 and 24, are outside their 48- and
                # 24-wide levels: level 0 alone is drawn
                assert f[1]["valid"] == f[2]["valid"] == 0 and f[1]["begin"] == (48, 40)
                continue
            assert f[1]["ntiles"] == 2 and f[2]["ntiles"] == 1
            assert 0 < f[2]["nu"] < f[1]["nu"] < 7679   # the coarse levels merge neighbours
    # the split G3 cases fit the register instance and the ring kernel
    assert all(c.n_max <= K.REG_POINTS for c in _kind("every_cell") if c.name.endswith("_split"))
    assert all(K.PATHS["ring"].admits(c) for c in _kind("every_cell") if c.geo in (K.G1, K.G2A, K.G2B))

    # ---- the one-workgroup path owns several tiles (the two-buffer pipeline past its first tile), with parts > ntx too
    p1, p321, p64 = K.PATHS["parts1"], K.PATHS["parts321"], K.PATHS["parts64"]
    for gname, tiles in (("G2a", 2), ("G2b", 3), ("G3", 4), ("G4", 6)):
        for c in (x for x in _kind("every_cell") if x.geo.name == gname):
            per = [f[0]["tiles_per_wg"] for f in K.reach(c, p1)]
            # (half a split scan may cover half the map)
            assert max(per) == tiles and (min(per) == tiles or (c.name.endswith("_split") and min(per) >= 2)), c.name
    assert all(f[0]["tiles_per_wg"] == 2 for f in K.reach(cases["every_G3_63_31"], p321))      # 4 tiles in 3 parts
    assert all(f[0]["tiles_per_wg"] == 2 and f[1]["tiles_per_wg"] == 1 for f in K.reach(cases["every_G4_48_40"], p321))
    assert p64.parts(1, 256) == [64] and p321.parts(3, 32) == [3, 2, 1] and p1.parts(3, 256) == [1, 1, 1]
    # the list split of one updating stream, on a partition (32 CUs) and on the whole device (256)
    assert K.PATHS["regs"].parts(3, 32) == [64, 32, 16] and K.PATHS["regs"].parts(3, 256) == [64, 64, 64]
    assert K.PATHS["split532"].parts(3, 32, U=40) == [5, 3, 2] and K.PATHS["regs"].parts(3, 32, U=40) == [4, 2, 1]

    # ---- star: every half-width that fits, both sides of a seam, a turned second update with duplicates
    for c in _kind("star"):
        f = K.reach(c)
        assert f[0][0]["nu"] == f[0][0]["n"] > 0 and f[1][0]["valid"] > 0
    f = K.reach(cases["star_G6x"])
    assert f[0][0]["da_max"] == 65 and f[0][0]["ntx"] == 4 and f[0][0]["nty"] == 5   # x 1983 .. 2113, y 15 .. 145

    # ---- edges
    for c in _kind("edges"):
        g, f = c.geo, K.reach(c)
        u0, u3 = c.updates[0], c.updates[3]
        for u in (u0, u3):
            e = u.ends
            assert e[:8] == [(0, e[0][1]), (g.sx - 1, e[1][1]), (e[2][0], 0), (e[3][0], g.sy - 1), (0, 0), (g.sx - 1, 0),
                             (0, g.sy - 1), (g.sx - 1, g.sy - 1)]
            assert [e[8][0], e[9][0], e[10][1], e[11][1]] == [-1, g.sx, -1, g.sy]          # one beyond: cancelled
            for i in range(12, 24, 3):                                                      # truncation toward zero
                assert e[i][0] == 0 and e[i + 1][1] == 0 and e[i + 2] == (0, 0), (c.name, i, e[i:i + 3])
            for i in range(25, 40):                                                         # NaN, inf, 1e10
                assert -1 in e[i] or max(e[i]) > 10 ** 9 or min(e[i]) < -10 ** 9, (c.name, i, e[i])
            assert e[40] == e[41] == u.begin                                                # begin == end
        # update 0 draws the 8 border cells and the 12 truncated ones; begin outside: nothing, the indices advance
        assert f[0][0]["valid"] in (20, 21) and f[0][0]["nu"] >= 8
        assert c.updates[1].begin[0] >= g.sx and c.updates[2].begin[0] == -2
        for k in (1, 2):
            assert f[k][0]["valid"] == 0
            # (G4's coarse levels truncate the pose's -2.75 / 2 + 0.5 into cell 0: they do draw)
            assert g.levels > 1 or f[k]["counters"] == dict(cells=0, rays=0, touched=0)
        assert u3.begin == (g.sx - 1, g.sy - 1) and f[3][0]["valid"] >= 19

    # ---- limit: da at the kernel's limit, long rays at small db, many tiles per workgroup on the list path
    for c in _kind("limit"):
        g, f = c.geo, K.reach(c, K.PATHS["regs"], ncu=32)
        lim = max(g.sx, g.sy) - 1
        assert lim == {"G5": 16384, "G5r": 16383, "G6": 4095}[g.name[:-1]]
        for k, fk in enumerate(f):
            assert fk[0]["da_max"] == lim and fk[0]["valid"] == fk[0]["n"] == fk[0]["nu"], (c.name, k)
            assert fk["counters"]["cells"] > c.da_sum[k] > 6 * lim
            assert fk[0]["tiles_per_wg"] >= 5 and fk[0]["ntiles"] > 64, (c.name, k, fk[0]["ntiles"])
        assert K.PATHS["regs"].admits(c) and (K.PATHS["ring"].admits(c) == (lim < 16384))
    assert max(f[0]["kmax"] for f in K.reach(cases["limit_G5ry"])) == 511      # rings above 255 (ring_split_w)
    assert max(f[0]["kmax"] for f in K.reach(cases["limit_G5rx"])) == 255

    # ---- values: every table entry under a free-only, a hit-only and a freed-then-hit cell
    t = K.value_table()
    for c in _kind("values"):
        f = K.reach(c)[0]
        for lvl in range(c.geo.levels):
            sx = c.geo.sx >> lvl
            seen = {}
            for off, what in f[lvl]["outcome"].items():
                seen.setdefault((K.VALUE_STRIDE[0] * (off % sx) + K.VALUE_STRIDE[1] * (off // sx)) % len(t), set()).add(what)
            need = {"free", "hit", "freed_hit"} if c.name.endswith("far_first") else {"free", "hit"}
            if lvl == 0:
                assert all(seen.get(i, set()) >= need for i in range(len(t))), (c.name, lvl, seen)
                assert f[lvl]["quad_full"] and f[lvl]["quad_part"] and f[lvl]["quad_nohit"] and f[lvl]["quad_hit"]

    # ---- sparse: stored quads with one, two and three cells drawn and payload NaNs beside them; the second update
    #      draws other cells of quads whose neighbours carry the first update's ordinals
    for c in _kind("sparse"):
        f = K.reach(c)
        q0 = f[0][0]["quads"]
        assert {len(v) for v in q0.values()} == {1, 2, 3} and f[0][0]["quad_full"] == 0
        assert len({k // (c.geo.sx * 32) for k in q0}) == -(-c.geo.sy // 32)      # in every tile row
        first = {o for v in q0.values() for o in v}
        q1 = f[1][0]["quads"]
        mixed = [k for k, v in q1.items() if k in q0 and len(v) < 4 and (set(q0[k]) - set(v))]
        assert len(mixed) >= c.geo.sy // 2 and any(set(v) - first for v in q1.values())

    # ---- many_distinct: nu = n at the boundary of the ballot's 64 groups and near the LDS budget
    for c in _kind("many_distinct"):
        f = K.reach(c)[0][0]
        assert f["nu"] == f["n"] == c.n_max and f["n"] in (4096, 4097, 4160, 10000)
        for p in ("lds", "parts1", "split532"):
            assert K.PATHS[p].admits(c) and K.PATHS[p].shmem_bytes(c) <= 65536
        assert not K.PATHS["regs"].admits(c) and not K.PATHS["ring"].admits(c)
    assert K.PATHS["lds"].shmem_bytes(cases["many_10000"]) == 4 * (K.UPD_FIXED_WORDS + 10000 + 4 * 160) > 60000

    # ---- G7: a box of more than MAX_BIN_TILES tiles
    fb = K.reach(cases["g7b_corners"])[0][0]
    assert fb["ntiles"] == 32 * 32 == K.MAX_BIN_TILES and ("binned", "g7b_corners") in K.plan()   # ... and of exactly that many
    f = K.reach(cases["g7_corners"])[0][0]
    assert f["ntiles"] == 33 * 33 > K.MAX_BIN_TILES and f["valid"] == 4

    # ---- the plan: every path row has its required cases
    plan = K.plan()
    rows = {p: {cases[c].kind for q, c in plan if q == p} for p in K.PATHS}
    for p, kinds in rows.items():
        assert {"every_cell", "edges", "values", "sparse"} <= kinds, p
    for p in ("regs", "lds", "parts1", "parts64", "split532"):
        assert (p, "limit_G5x") in plan and (p, "limit_G5y") in plan
    for p in ("ring", "ring_p1", "ring_p4", "ring_p64"):
        assert (p, "limit_G5rx") in plan and (p, "limit_G5ry") in plan
    assert "many_distinct" in rows["lds"] and "many_distinct" in rows["parts1"] and ("binned", "g7_corners") in plan


def test_batch_preconditions():
    """The batch's six streams through the oracles: on some step both did_update values occur; the oracle's update of
    every step equals the plain statement's from the oracle's pose."""
    scans, hints = K.batch_scans()
    assert sorted(len(s) for s in scans)[:2] == [0, 0] and len({len(s) for s in scans}) == 5
    oras = [K.make_oracle(K.G4) for _ in scans]
    plains = [K.plain_map(K.G4) for _ in scans]
    for o in oras:
        o.set_thresholds(0.4, 0.9)
    mixed = 0
    for t in range(3):
        did = []
        for s, (o, pl) in enumerate(zip(oras, plains)):
            pose, _, d = o.process(scans[s], hint=hints[t, s])
            did.append(d)
            assert np.isfinite(pose).all()
            if d:
                pl.store_container(scans[s])
                pl.update_by_scan(scans[s], pose)
                for lvl in range(3):
                    np.testing.assert_array_equal(o.level(lvl)[0].view(np.int32), pl.level(lvl)[0].view(np.int32))
                    np.testing.assert_array_equal(o.level(lvl)[1], pl.level(lvl)[1])
        assert t > 0 or all(did)
        mixed += len(set(did)) == 2
    assert mixed >= 1
