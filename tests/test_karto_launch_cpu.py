"""The Karto host policy (csrc/karto_internal.h) on the CPU: the options parser, the matcher's geometry, what a chunk
of matches launches, and the occupancy-grid rebuild's workgroups per tile.

tests/cpp/karto_launch_check.cpp includes the header the library is built from and prints, for a line of knobs, a
laser, parameters and a batch shape, the parsed options, the geometry and the plans.  This file holds the geometry to
oracle/karto_oracle.c (ko_grid_info, ko_kernel) on every parameter set of tests/ref/karto_cases.py, reaches each
refusal of kt_geometry by one directed input, and holds the plan to the kernel that the ids and docstrings of
tests/test_karto_paths_gpu.py name for its rows -- so a drift shows here and not as a GPU test that passes on another
kernel than its id says.

Every line sent is also left in tests/cpp/build/karto_launch_lines.txt: `make -C tests/cpp asan` runs a build of the
same program with -fsanitize=address,undefined over them.
"""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import oracle as O

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "ref"))
import karto_cases as K  # noqa: E402
import test_karto_paths_gpu as G  # noqa: E402  (its BUILDS and KNOBS rows; nothing of it runs here)

CPP = os.path.join(HERE, "cpp")
EXE = os.path.join(CPP, "build", "karto_launch_check")
LINES = os.path.join(CPP, "build", "karto_launch_lines.txt")
NONE, BINNED, PER_MATCH, PER_BASE = 0, 1, 2, 3   # enum KtAddScans: -, kt_addscans_kernel, kt_build_kernel<0, 8>, <0, 4>
CLEAR_NONE, CLEAR_TILES, CLEAR_FOOTPRINT = 0, 1, 2   # enum KtClear: -, kt_clear_tiles_kernel, kt_build_kernel<1, 4>
BUILD_DEFAULT, BUILD_CAS, BUILD_PER_BASE = 0, 1, 2   # enum KtBuild


@pytest.fixture(scope="module")
def check():
    subprocess.check_call(["make", "-s", "-C", CPP, "build/karto_launch_check"])
    open(LINES, "w").close()

    def run(lines):
        text = "\n".join(lines) + "\n"
        with open(LINES, "a") as f:
            f.write(text)
        out = subprocess.run([EXE], input=text, capture_output=True, text=True, check=True).stdout.splitlines()
        assert len(out) == len(lines)
        return [json.loads(o) for o in out]

    return run


def _knobs(env):
    return " ".join(f"{k}={v}" for k, v in dict(env).items())


def line(env=(), lz=None, p=None, max_matches=1, max_base=1, count=1, pas=0):
    lz, p = lz or K.laser(), p or K.params()
    nums = [getattr(lz, f) for f, _ in O.KtLaser._fields_[:5]] + [getattr(p, f) for f, _ in O.KtParams._fields_[:11]]
    return f"{_knobs(env)} | {' '.join(repr(v) for v in nums)} {max_matches} {max_base} {count} {pas}"


def split_line(env, num_cus, ntiles, count):
    return f"{_knobs(env)} | split {num_cus} {ntiles} {count}"


def ceil8(v):
    return (v + 7) // 8 * 8


def test_constants(check):
    c = json.loads(subprocess.run([EXE, "constants"], capture_output=True, text=True, check=True).stdout)
    assert c == {"KT_THREADS": 256, "KT_MAX_READINGS": 4096, "KT_FINE_MAX_ANG": 64, "KT_MAX_NXY": 1024, "KT_OCC": 100,
                 "KT_AS_WAVES": 8, "KT_AS_MAX_TILES": 2048, "KT_AS_MAX_BASE": 1024, "KT_FINE_THREADS": 256,
                 "KG_MAX_SPLIT": 32, "sizeof_KtGeom": 280}


# ------------------------------------------------------------------------------------------ geometry
def parameter_sets():
    """(name, laser, params) of everything tests/ref/karto_cases.py produces."""
    sets = [("default", K.laser(), K.params()), ("loop", K.laser(), K.params(loop=True))]
    sets += [(f"smear_{k}", K.laser(), K.smear_params(k)) for k in K.SMEAR_KEYS]
    sets += [(c.name, c.laser, c.params) for c in [K.dense()] + list(K.expansion().values())]
    sets += [(c.name, c.laser, c.params) for n in K.SHORT_N for c in K.short(n)[:1]]
    sets += [(c.name, c.laser, c.params) for c in K.headings()[:1] + list(K.degenerate().values())]
    return sets


def test_geometry_equals_the_oracle(check):
    """kt_get_grid_info's first nine words equal ko_grid_info's, the smear kernel ko_kernel's byte for byte."""
    sets = parameter_sets()
    assert {s[2].use_response_expansion for s in sets} == {0, 1} and {s[1].n_readings for s in sets} >= {1, 257, 1081, 4096}
    got = check([line((), lz, p) for _, lz, p in sets])
    ksizes = set()
    for (name, lz, p), g in zip(sets, got):
        want = O.karto_grid_info(p, lz)
        assert g["grid_info"][:9] == list(want.values()), name
        assert g["grid_info"][9] == g["max_poses"] == g["nxy"] ** 2 * g["nang"][g["npass"] - 1], name
        k = np.zeros(want["ksize"] ** 2, np.uint8)
        assert O.karto_lib().ko_kernel(p, lz, O._fp(k), k.size) == k.size, name
        assert bytes.fromhex(g["kernel"]) == k.tobytes(), name
        assert (g["n"], g["npass"], g["fn"]) == (lz.n_readings, 4 if p.use_response_expansion else 1, 3), name
        ksizes.add(g["ksize"])
    assert ksizes == {3, 13, 15, 17, 35, 41}


def test_geometry_refusals(check):
    """Each refusal of kt_geometry by one directed input, in the function's order.  Two of its checks cannot fire:
    * "smear kernel wider than 41 cells": the check before it admits smear <= 10 * res only, so 2 * smear / res is at
      most 20 (1 + 2^-52) and rounds to a half of 20 at most, i.e. 41 cells;
    * "fine search must be 3x3 positions": foff = (2 * res) * 0.5 is res exactly, foff * 2 / res is 2 exactly and
      fn = 3 for every finite 2 * res.
    Both stay in the code as guards of what the kernels' LDS arrays assume."""
    D = K.D
    rows = [
        (K.laser(), K.params(resolution=0.0), "ScanMatcher::Create rejects these parameters"),
        (K.laser(), K.params(resolution=-0.01), "ScanMatcher::Create rejects these parameters"),
        (K.laser(0), K.params(), "n_readings must be in [1, 4096]"),
        (K.laser(4097), K.params(), "n_readings must be in [1, 4096]"),
        (K.laser(), K.params(coarse_angle_resolution=0.0), "angle offsets / resolutions must be > 0"),
        (K.laser(thr=250.0), K.params(resolution=0.005), "correlation grid larger than 2^31 cells"),
        (K.laser(), K.params(smear_deviation=0.004), "smear deviation must be between 0.5 and 10 resolutions"),
        (K.laser(), K.params(smear_deviation=0.101), "smear deviation must be between 0.5 and 10 resolutions"),
        (K.laser(), K.params(smear_deviation=0.0999), "smear kernel has an off-centre value of 100"),
        (K.laser(), K.params(search_size=20.48), "coarse search wider than 1024 positions"),
        (K.laser(), K.params(fine_search_angle_offset=0.02 * D), "fine search has more than 64 angles"),
        (K.laser(), K.params(coarse_angle_resolution=0.0001, fine_search_angle_offset=0.0001),
         "coarse search has more than 4096 angles"),
        (K.laser(), K.params(search_size=20.46, coarse_angle_resolution=0.2 * D), "coarse search window larger than 2e8 poses"),
    ]
    got = check([line((), lz, p) for lz, p, _ in rows])
    for (lz, p, want), g in zip(rows, got):
        assert g.get("error", "").startswith(want), (want, g)
    # the neighbours that pass: 4096 readings, a kernel of 41 cells whose ring is 99, 1024 positions, 64 fine angles
    ok = check([line((), K.laser(4096), K.params()), line((), K.laser(), K.params(smear_deviation=0.099)),
                line((), K.laser(), K.params(search_size=20.46)),
                line((), K.laser(), K.params(fine_search_angle_offset=2 * D / 63))])
    assert [g.get("error") for g in ok] == [None] * 4
    assert (ok[1]["ksize"], ok[2]["nxy"], ok[3]["fnang"]) == (41, 1024, 64)


# ------------------------------------------------------------------------------------------ the plan
def test_addscans_kernel_of_each_build_row(check):
    """test_grid_byte_for_byte's BUILDS on its own shapes (K.smear_batch(M): 6 base scans at most, every smear key),
    and 127 against 128 matches under each setting."""
    assert G.BUILDS == [(3, None), (128, None), (128, "cas"), (128, "per_base")]
    want_of = {(3, None): PER_BASE, (128, None): BINNED, (128, "cas"): PER_MATCH, (128, "per_base"): PER_BASE}
    mb = K.smear_batch(3).max_base
    assert mb == 6
    rows = [(M, b, k) for M, b in G.BUILDS for k in K.SMEAR_KEYS]
    rows += [(M, b, 13) for M in (127, 128) for b in (None, "cas", "per_base")]
    got = check([line({"SLAM2D_KT_BUILD": b} if b else {}, K.laser(), K.smear_params(k), M, mb, M) for M, b, k in rows])
    for (M, b, k), g in zip(rows, got):
        want = want_of[(M, b)] if M != 127 else PER_BASE
        assert g["add"] == want, (M, b, k, g)
        assert g["slots"] == M
        if want == BINNED:       # kt_addscans_kernel: one 512-thread workgroup per match; the clear by dirty tiles
            assert (g["add_grid"], g["add_block"]) == (M, 512)
            assert (g["clear"], g["clear_grid_x"], g["clear_grid_y"]) == (CLEAR_TILES, M, 4)
        elif want == PER_MATCH:  # kt_build_kernel<0, 8>: one 512-thread workgroup per match
            assert (g["add_grid"], g["add_block"]) == (M, 512)
            assert (g["clear"], g["clear_grid_x"], g["clear_grid_y"]) == (CLEAR_FOOTPRINT, ceil8(M) * mb, 1)
        else:                    # kt_build_kernel<0, 4>: one workgroup per (match of an 8-group, base scan)
            assert (g["add_grid"], g["add_block"]) == (ceil8(M) * mb, 256)
            assert (g["clear"], g["clear_grid_x"], g["clear_grid_y"]) == (CLEAR_FOOTPRINT, ceil8(M) * mb, 1)
        assert (g["fine_grid"], g["fine_block"]) == (M, 256)
    # no base scans at all: neither a build nor a clear (test_degenerate_sets' all_tie cases run on max_base 3)
    g, = check([line((), max_matches=128, max_base=0, count=128)])
    assert (g["add"], g["clear"], g["add_grid"], g["clear_grid_x"]) == (NONE, CLEAR_NONE, 0, 0)
    # MatchScan (one match) with 32 base scans: test_many_base_scans_results' kt_build_kernel<0, 4>
    g, = check([line((), max_matches=1, max_base=32, count=1)])
    assert (g["add"], g["add_grid"]) == (PER_BASE, 8 * 32)


def test_binned_eligibility(check):
    """The binned kernel's LDS tables hold 2048 tiles and 1024 base scans: past either, and under either CAS setting,
    a batch of 128 takes kt_build_kernel<0, 8> and the context needs no scratch."""
    wide = K.laser(thr=80.0)   # 3361 cells + border: 53 x 53 tiles
    rows = [((), K.laser(), K.params(loop=True), 1024, 1, BINNED), ((), K.laser(), K.params(loop=True), 1025, 0, PER_MATCH),
            ((), wide, K.params(loop=True), 6, 0, PER_MATCH), ({"SLAM2D_KT_BUILD": "cas"}, K.laser(), K.params(), 6, 0, PER_MATCH),
            ({"SLAM2D_KT_BUILD": "per_base"}, K.laser(), K.params(), 6, 0, PER_BASE),
            ({"SLAM2D_KT_BUILD": "junk"}, K.laser(), K.params(), 6, 1, BINNED)]
    got = check([line(env, lz, p, 128, mb, 128) for env, lz, p, mb, _, _ in rows])
    for (env, lz, p, mb, eligible, add), g in zip(rows, got):
        assert (g["binned_eligible"], g["add"]) == (eligible, add), (env, mb, g)
    assert got[2]["ntiles"] == 53 * 53 > 2048 >= got[0]["ntiles"]
    # the edge on square grids: 45 x 45 = 2025 <= 2048 < 46 x 46 tiles
    a, b = check([line((), K.laser(thr=67.0), K.params(loop=True), 128, 6, 128),
                  line((), K.laser(thr=69.0), K.params(loop=True), 128, 6, 128)])
    assert (a["ntiles"], a["add"], b["ntiles"], b["add"]) == (45 * 45, BINNED, 46 * 46, PER_MATCH)


def test_prepare_lds(check):
    """kt_prepare_kernel: 24 bytes per reading; test_dense_scan_results' 4096 beams need the attribute call, 1081 do
    not, and the edge is n_readings 2730 | 2731."""
    rows = [(1081, 0), (4096, 1), (2730, 0), (2731, 1), (1, 0)]
    got = check([line((), K.laser(n, thr=20.0)) for n, _ in rows])
    for (n, attr), g in zip(rows, got):
        assert (g["prepare_lds"], g["prepare_attr"]) == (24 * n, attr), (n, g)
    assert 24 * 2730 <= 65536 < 24 * 2731 and got[1]["prepare_lds"] == 98304
    c = K.dense()
    g, = check([line((), c.laser, c.params, 1, 5, 1)])
    assert g["prepare_attr"] == 1 and c.laser.n_readings >= 2731


def test_select_instance(check):
    """kt_select_kernel<1024> above 512 coarse positions: the default window (16 x 16) and loop21 (441) take <256>,
    all_tie_81 (6561) <1024>; the edge lies between 22 x 22 = 484 and 23 x 23 = 529."""
    deg = K.degenerate()
    rows = [(K.params(), 16, 256), (K.smear_params("loop"), 21, 256), (deg["all_tie_21"].params, 21, 256),
            (deg["all_tie_81"].params, 81, 1024), (K.params(loop=True, search_size=2.1), 22, 256),
            (K.params(loop=True, search_size=2.2), 23, 1024)]
    got = check([line((), K.laser(), p, 1, 3, 1) for p, _, _ in rows])
    for (p, nxy, threads), g in zip(rows, got):
        assert (g["nxy"], g["select_threads"]) == (nxy, threads), (nxy, g)
        assert g["nang"][0] == 21


def test_knob_rows(check):
    """test_knobs_keep_results' KNOBS on its two batches: 130 sequential matches of 8 base scans at most (default
    parameters) and 16 loop matches of 6 on the 21 x 21 window."""
    assert G.KNOBS == [("SLAM2D_KT_SLOTS", "48"), ("SLAM2D_KT_AG", "3"), ("SLAM2D_KT_AG", "21"), ("SLAM2D_KT_TW", "32"),
                       ("SLAM2D_KT_TW", "64"), ("SLAM2D_POISON", "1")]
    seq = lambda env, count=130: line(env, K.laser(), K.params(), 130, 8, count)   # noqa: E731
    loop = lambda env: line(env, K.laser(), K.smear_params("loop"), 16, 6, 16)      # noqa: E731
    base_s, base_l = check([seq({}), loop({})])
    assert (base_s["slots"], base_s["add"], base_s["coarse_ag"], base_s["coarse_blocks"]) == (130, BINNED, 1, 136 * 21)
    assert (base_l["add"], base_l["nxy"], base_l["ctx"], base_l["cty"], base_l["coarse_blocks"]) == (PER_BASE, 21, 2, 2, 16 * 4 * 21)
    # SLOTS=48: chunks of 48, 48, 34 (kt_run_batch's loop), each below 128 matches: kt_build_kernel<0, 4>
    g, = check([seq({"SLAM2D_KT_SLOTS": "48"})])
    assert g["slots"] == 48
    chunks = [min(g["slots"], 130 - c0) for c0 in range(0, 130, g["slots"])]
    assert chunks == [48, 48, 34]
    for cnt, g in zip(chunks, check([seq({"SLAM2D_KT_SLOTS": "48"}, cnt) for cnt in chunks])):
        assert (g["add"], g["add_grid"], g["coarse_blocks"]) == (PER_BASE, ceil8(cnt) * 8, ceil8(cnt) * 21)
    # AG: angles per workgroup, clamped to [1, nang] when planned
    for ag, want_ag, groups in (("3", 3, 7), ("21", 21, 1), ("0", 1, 21), ("-4", 1, 21), ("99", 21, 1), ("4", 4, 6)):
        s, l = check([seq({"SLAM2D_KT_AG": ag}), loop({"SLAM2D_KT_AG": ag})])
        assert s["angle_group"] == l["angle_group"] == int(ag)
        assert (s["coarse_ag"], s["coarse_blocks"]) == (want_ag, ceil8(130) * 1 * 1 * groups), (ag, s)
        assert (l["coarse_ag"], l["coarse_blocks"]) == (want_ag, ceil8(16) * 2 * 2 * groups), (ag, l)
    # a later pass of response expansion has its own angle count (41, 61, 81)
    ex = K.expansion()[50]
    got = check([line({"SLAM2D_KT_AG": "30"}, ex.laser, ex.params, 1, 1, 1, pas) for pas in range(4)])
    assert [(g["nang"][pas], g["coarse_ag"], g["coarse_blocks"]) for pas, g in enumerate(got)] == \
        [(21, 21, 8), (41, 30, 16), (61, 30, 24), (81, 30, 24)]
    # TW: 32 x 8 and 64 x 4 position tiles
    for tw, clw, tx, ty in (("16", 2, 16, 16), ("32", 3, 32, 8), ("64", 4, 64, 4)):
        s, l = check([seq({"SLAM2D_KT_TW": tw}), loop({"SLAM2D_KT_TW": tw})])
        for g, nxy in ((s, 16), (l, 21)):
            assert (g["tile_w"], g["clw"], g["ctx"], g["cty"]) == (int(tw), clw, -(-nxy // tx), -(-nxy // ty)), (tw, g)
            assert g["coarse_blocks"] == ceil8(g["fine_grid"]) * g["ctx"] * g["cty"] * 21
    assert (l["ctx"], l["cty"]) == (1, 6)
    g, = check([seq({"SLAM2D_POISON": "1"})])
    assert g["poison"] == 1 and {k: v for k, v in g.items() if k != "poison"} == {k: v for k, v in base_s.items() if k != "poison"}


def test_coarse_launch_refusal(check):
    """More than 2^31 - 1 workgroups: 65535 matches on a 1024 x 1024 window (8192 groups x 64 x 64 tiles x 21)."""
    p = K.params(search_size=20.46)
    small, big = check([line((), K.laser(), p, 65535, 1, 6), line((), K.laser(), p, 65535, 1, 65535)])
    assert (small["nxy"], small["ctx"], small["cty"]) == (1024, 64, 64)
    assert (small["coarse_blocks"], small["coarse_refused"]) == (8 * 4096 * 21, None)
    assert big["coarse_blocks"] == 65536 * 4096 * 21 > 2**31 - 1
    assert big["coarse_refused"] == "coarse launch too large: lower the batch size"
    # the largest launch that passes: 2^31 - 1 >= 24960 * 4096 * 21 = 2146959360, and 24968 groups are too many
    a, b = check([line((), K.laser(), p, 65535, 1, 24960), line((), K.laser(), p, 65535, 1, 24961)])
    assert (a["coarse_refused"], b["coarse_blocks"], b["coarse_refused"] is None) == (None, 24968 * 4096 * 21, False)


# ------------------------------------------------------------------------------------------ the parser
def test_parser(check):
    """One row per knob: unset, the empty string, valid values, malformed ones.  A number that is not one whole
    decimal integer is refused (kt_create / kg_create: EINVAL with this message), not read the way atoi would."""
    TW, AG = "SLAM2D_KT_TW must be 16, 32 or 64", "SLAM2D_KT_AG must be an integer"
    SL, PO = "SLAM2D_KT_SLOTS must be an integer", "SLAM2D_POISON must be an integer"
    table = [
        ("SLAM2D_KT_TW", "tile_w", {None: 16, "": TW, "16": 16, "32": 32, "64": 64, "abc": TW, "48": TW, "32x": TW, "0": TW}),
        ("SLAM2D_KT_AG", "angle_group", {None: 1, "": AG, "1": 1, "3": 3, "0": 0, "-2": -2, "99": 99, "3.5": AG,
                                         "seven": AG, "3,4": AG, "99999999999": AG}),
        ("SLAM2D_KT_SLOTS", "slots_knob", {None: 0, "": SL, "48": 48, "0": 0, "-1": -1, "1000": 1000, "48k": SL}),
        ("SLAM2D_KT_SLOTS", "slots", {None: 130, "48": 48, "1": 1, "0": 130, "-1": 130, "130": 130, "1000": 130}),
        ("SLAM2D_KT_BUILD", "build", {None: BUILD_DEFAULT, "": BUILD_DEFAULT, "cas": BUILD_CAS, "per_base": BUILD_PER_BASE,
                                      "CAS": BUILD_DEFAULT, "binned": BUILD_DEFAULT}),
        ("SLAM2D_POISON", "poison", {None: 0, "": PO, "1": 1, "0": 0, "-1": 1, "2": 1, "yes": PO}),
    ]
    for knob, field, rows in table:
        got = check([line({} if v is None else {knob: v}, max_matches=130, max_base=8, count=130) for v in rows])
        assert [g.get(field, g.get("error")) for g in got] == list(rows.values()), (knob, field, list(rows))
    KG = "SLAM2D_KG_SPLIT must be an integer"
    rows = {None: 0, "": KG, "4": 4, "0": 0, "-3": -3, "40": 40, "x": KG, "4,8": KG}
    got = check([split_line({} if v is None else {"SLAM2D_KG_SPLIT": v}, 256, 100, 640) for v in rows])
    assert [g.get("force_split", g.get("error")) for g in got] == list(rows.values())


# ------------------------------------------------------------------------------------------ kg_split_rule
def test_kg_split_rule(check):
    """Workgroups per tile of the occupancy-grid rebuild, (forced, CUs, tiles, scans) -> split."""
    rows = [
        ("5", 256, 100, 640, 5), ("32", 256, 100, 640, 32), ("40", 256, 100, 640, 32),   # forced; forced above 32
        ("1", 256, 1, 5000, 1), ("0", 256, 100, 640, 16), ("-3", 256, 100, 640, 16),     # <= 0: the rule
        (None, 256, 1024, 1000, 1), (None, 256, 5000, 1000, 1),    # the tiles alone give 4 workgroups per CU
        (None, 256, 1023, 1000, 2), (None, 256, 512, 1000, 2),
        (None, 256, 400, 1000, 4),                                 # 3 -> 4
        (None, 256, 256, 1000, 4),
        (None, 256, 205, 1000, 8), (None, 256, 200, 1000, 8), (None, 256, 147, 1000, 8),   # 5, 6, 7 -> 8
        (None, 256, 128, 1000, 8), (None, 256, 100, 1000, 16),     # 8; 11 -> 16
        (None, 256, 50, 1000, 24),                                 # 21 -> 24
        (None, 256, 100, 64, 2), (None, 256, 100, 1, 1), (None, 256, 100, 32, 1), (None, 256, 100, 33, 2),   # >= 32 scans per workgroup
        (None, 256, 100, 96, 4), (None, 256, 100, 160, 8), (None, 256, 100, 352, 16),
        (None, 256, 40, 5000, 32), (None, 256, 10, 5000, 32), (None, 256, 1, 100000, 32),   # 26 -> 32; 103 and 1024: the cap
        (None, 32, 128, 1000, 1), (None, 32, 64, 1000, 2), (None, 32, 20, 1000, 8), (None, 32, 16, 1000, 8),
        (None, 32, 1, 10000, 32), (None, 32, 1, 100, 4),
    ]
    got = check([split_line({} if f is None else {"SLAM2D_KG_SPLIT": f}, cus, nt, cnt) for f, cus, nt, cnt, _ in rows])
    assert [g["split"] for g in got] == [r[4] for r in rows], [(r, g) for r, g in zip(rows, got) if g["split"] != r[4]]
