"""Every kernel path of the Karto correlative matcher (csrc/karto_kernels.hip) against oracle/karto_oracle.c, bit for
bit: the correlation grid byte for byte (kt_copy_grid_device against ko_build_grid), the whole coarse response volume
(the exchange words against ko_coarse_responses) and the results (mean, covariance, response) -- over every smear
branch, every AddScans kernel, long / short / degenerate scans, late response expansion and the run-time knobs.  The
inputs come from tests/ref/karto_cases.py; test_path_case_preconditions (tests/test_karto_cpu.py) asserts on the same
inputs the property that makes each case reach its path.  No tolerances anywhere."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

import oracle as O
from slam2d import karto

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "ref"))
import karto_cases as K  # noqa: E402

pytestmark = pytest.mark.gpu


def _kl(l):
    return karto.KtLaser(*[getattr(l, f) for f, _ in karto.KtLaser._fields_])


def _kp(p):
    return karto.KtParams(*[getattr(p, f) for f, _ in karto.KtParams._fields_])


def _same(gpu_out, ora_out):
    gm, gc, gr = gpu_out
    om, oc, orr = ora_out
    np.testing.assert_array_equal(gm, om)
    np.testing.assert_array_equal(gc, oc)
    assert gr == orr


_ORACLE = {}


def _oracle_match(key, case, **kw):
    """karto_match of a case, computed once per session and shared by the tests that need it."""
    k = (key, tuple(sorted(kw.items())))
    if k not in _ORACLE:
        _ORACLE[k] = case.match(**kw)
    return _ORACLE[k]


def _match_scan(sm, case, **kw):
    pen, ref = kw.get("penalize", case.penalize), kw.get("refine", case.refine)
    return sm.MatchScan(case.q_ranges, case.q_pose, case.b_ranges, case.b_poses, pen, ref)


def _single(case, max_base=None):
    B = len(case.b_ranges)
    mb = max(B, 1) if max_base is None else max_base
    return karto.ScanMatcher(_kl(case.laser), _kp(case.params), max_matches=1, max_scans=mb + 1, max_base=mb)


class _Pooled:
    """A K.Batch on the device: the pool in a ScanMatcher of `count` slots and the index arrays."""

    def __init__(self, batch, lz, p):
        import torch

        self.torch, self.batch, self.lz, self.p = torch, batch, lz, p
        S = batch.pool_ranges.shape[0]
        self.sm = karto.ScanMatcher(_kl(lz), _kp(p), max_matches=batch.count, max_scans=S, max_base=batch.max_base)
        self.hs = torch.cuda.current_stream().cuda_stream
        self.pr = torch.tensor(batch.pool_ranges, dtype=torch.float64, device="cuda")
        self.pp = torch.tensor(batch.pool_poses, dtype=torch.float64, device="cuda")
        self.sm.set_scans_device(0, S, self.pr.data_ptr(), self.pp.data_ptr(), hip_stream=self.hs)
        self.q, self.beg, self.idx = (torch.tensor(a, device="cuda") for a in (batch.query, batch.begin, batch.index))
        self.nbytes = batch.count * C.sizeof(karto.KtResult)

    def run(self, penalize=True, refine=True):
        res = self.torch.zeros(self.nbytes, dtype=self.torch.uint8, device="cuda")
        self.sm.match_batch_device(self.batch.count, self.q.data_ptr(), self.beg.data_ptr(), self.idx.data_ptr(),
                                   res.data_ptr(), penalize, refine, hip_stream=self.hs)
        self.torch.cuda.synchronize()
        return karto.results_from_bytes(res.cpu().numpy())

    def begin(self, penalize=True):
        """kt_match_sharded_begin_device as the only shard: the grids are built and the exchange words exported."""
        M = self.batch.count
        self.x = self.torch.full((M, self.sm.exchange_words()), -1, dtype=self.torch.int64, device="cuda")
        self.sm.match_sharded_begin_device(M, self.q.data_ptr(), self.beg.data_ptr(), self.idx.data_ptr(), 0, 1,
                                           self.x.data_ptr(), penalize, hip_stream=self.hs)
        self.torch.cuda.synchronize()
        return self.x.cpu().numpy()

    def end(self, penalize=True, refine=True):
        res = self.torch.zeros(self.nbytes, dtype=self.torch.uint8, device="cuda")
        self.sm.match_sharded_end_device(self.batch.count, self.beg.data_ptr(), self.idx.data_ptr(), self.x.data_ptr(),
                                         res.data_ptr(), penalize, refine, hip_stream=self.hs)
        self.torch.cuda.synchronize()
        return karto.results_from_bytes(res.cpu().numpy())

    def case(self, i, **kw):
        return self.batch.case(i, self.lz, self.p, **kw)


def _same_result(out, i, ora):
    assert out["status"][i] == 0
    _same((out["mean"][i], out["covariance"][i].reshape(3, 3), out["response"][i]), ora)


def _check_grids(pb, slots, key):
    """Between begin and end: the device grid of each slot equals ko_build_grid byte for byte; after end: all zero,
    and the results equal karto_match."""
    pb.begin()
    for i in slots:
        c = pb.case(i)
        want = O.karto_build_grid(c.laser, c.params, c.q_pose, c.b_ranges, c.b_poses)
        got = pb.sm.grid(i)
        assert got.shape == want.shape and want.any()
        np.testing.assert_array_equal(got, want, err_msg=f"slot {i}")
    out = pb.end()
    for i in slots:
        assert not pb.sm.grid(i).any(), f"slot {i} not cleared"
        _same_result(out, i, _oracle_match((key, i), pb.case(i)))


# ------------------------------------------------------------------------------------------ grid, byte for byte
# AddScans kernels: M = 3 kt_build_kernel<0, 4>; M = 128 kt_addscans_kernel (binned, the default);
# SLAM2D_KT_BUILD=cas kt_build_kernel<0, 8> (one workgroup per match); =per_base kt_build_kernel<0, 4> at 128
BUILDS = [(3, None), (128, None), (128, "cas"), (128, "per_base")]


@pytest.mark.parametrize("M,build", BUILDS, ids=["m3", "m128_binned", "m128_cas", "m128_per_base"])
@pytest.mark.parametrize("smear", K.SMEAR_KEYS)
def test_grid_byte_for_byte(gpu, monkeypatch, smear, M, build):
    """Smear kernels 3 / 13 / 15 / 17 / 35 / 41 cells and the loop matcher's 3 at 0.05 m, through each AddScans
    kernel: kt_group's per-lane cell tables (ks <= 15) and lane-strided smear (ks > 15); kt_addscans_kernel's dword
    render (ks <= 13), kt_render_items<4> (ks = 15) and bounds-tested branch (ks > 15; half 17 / 20 of ks 35 / 41
    exceeds the 16-cell LDS margin).  Preconditions: the ksize of each smear value."""
    if build:
        monkeypatch.setenv("SLAM2D_KT_BUILD", build)
    pb = _Pooled(K.smear_batch(M), K.laser(), K.smear_params(smear))
    assert pb.sm.info["ksize"] == (3 if smear == "loop" else smear)
    _check_grids(pb, sorted({0, M // 2, M - 1}), ("smear", smear, M))


@pytest.mark.parametrize("smear", [13, 41])
def test_grid_many_base_scans_second_pass(gpu, smear):
    """32 / 31 / 30 base scans per match at M = 128 (binned): more than KT_AS_ITEMS = 15360 footprint items, so
    kt_addscans_kernel takes further passes and its `was` branch re-reads the tiles an earlier pass wrote -- with
    the dword render (ks 13) and the bounds-tested branch (ks 41).  Precondition (asserted per checked match in
    test_path_case_preconditions): the valid in-ROI points alone exceed 15360."""
    b = K.many_base_batch()
    pb = _Pooled(b, K.laser(), K.smear_params(smear))
    _check_grids(pb, [0, b.count // 2, b.count - 1], ("many", smear))


# ------------------------------------------------------------------------------------------ coarse volume
def _check_volume(x, case, penalize, nxy, nA):
    """Exchange words [best bits, ERANGE, posmax[nxy^2], responses[nA][nxy^2]] against ko_coarse_responses
    [y, x, angle]: every pose's response, the per-position maximum and the best."""
    want = O.karto_coarse_responses(case.laser, case.params, case.q_ranges, case.q_pose, case.b_ranges, case.b_poses,
                                    nxy, nA, penalize=penalize)
    assert x.shape[0] == 2 + nxy * nxy * (1 + nA) and x[1] == 0
    resp = x[2 + nxy * nxy:].view(np.float64).reshape(nA, nxy, nxy).transpose(1, 2, 0)
    np.testing.assert_array_equal(resp.view(np.int64), np.ascontiguousarray(want).view(np.int64))
    posmax = x[2:2 + nxy * nxy].view(np.float64).reshape(nxy, nxy)
    np.testing.assert_array_equal(posmax, want.max(axis=2))
    assert x[:1].view(np.float64)[0] == want.max()
    return want


@pytest.mark.parametrize("penalize", [True, False])
@pytest.mark.parametrize("window", ["sequential", "loop21", "ks41", "dense"])
def test_coarse_volume_every_pose(gpu, window, penalize):
    """The whole coarse window, not only its argmax: the default sequential window (16 x 16 x 21), the loop window
    at search_size 2.0 (21 x 21 x 21: two tiles per axis), ksize 41, and the dense scan -- whose 3633 points at a
    response of 0.946 pass 65535 per packed 16-bit lane unless kt_coarse_kernel flushes every 504 points per wave
    (precondition in test_path_case_preconditions: max_response * npts * 25 > 65535 and npts > 2045)."""
    if window == "dense":
        b, lz, p, nxy = K.Batch(*_batch_of(K.dense())), K.dense().laser, K.dense().params, 16
    elif window == "loop21":
        b, lz, p, nxy = K.loop_batch(16, 6), K.laser(), K.smear_params("loop"), 21
    else:
        b, lz, p, nxy = K.smear_batch(3), K.laser(), K.smear_params(41 if window == "ks41" else 13), 16
    pb = _Pooled(b, lz, p)
    x = pb.begin(penalize)
    assert (x >= 0).all()
    for i in sorted({0, b.count - 1}):
        want = _check_volume(x[i], pb.case(i), penalize, nxy, 21)
        assert want.max() > 0.1  # a window with content
    out = pb.end(penalize, True)
    for i in sorted({0, b.count - 1}):
        _same_result(out, i, _oracle_match((window, i), pb.case(i), penalize=penalize))


def _batch_of(case):
    """A single Case as a pooled batch of one match: slot 0 the query, then its base scans."""
    B = len(case.b_ranges)
    return (np.concatenate([case.q_ranges[None], case.b_ranges]), np.concatenate([case.q_pose[None], case.b_poses]),
            np.zeros(1, np.int32), np.array([0, B], np.int32), np.arange(1, B + 1, dtype=np.int32), B)


# ------------------------------------------------------------------------------------------ results, MatchScan path
@pytest.mark.parametrize("penalize,refine", [(True, True), (True, False), (False, True)])
def test_dense_scan_results(gpu, penalize, refine):
    """4096 beams, 3633 valid points: kt_prepare_kernel with 96 KB of dynamic LDS (n_readings >= 2731, the
    hipFuncSetAttribute branch of kt_create), kt_coarse_kernel's 16-bit flush, and all four register rounds of
    kt_fine_kernel (npts > 3072; 1081 beams use two), refine on and off."""
    c = K.dense()
    sm = _single(c)
    for _ in range(2):  # the slot is reused: the 16 MB grid must come back clean
        _same(_match_scan(sm, c, penalize=penalize, refine=refine),
              _oracle_match("dense", c, penalize=penalize, refine=refine))
    assert not sm.grid(0).any()


def test_many_base_scans_results(gpu):
    """32 base scans through MatchScan (kt_build_kernel<0, 4>, one workgroup per base scan)."""
    b = K.many_base_batch()
    c = b.case(0, K.laser(), K.params())
    _same(_match_scan(_single(c), c), _oracle_match((("many", 13), 0), c))


@pytest.mark.parametrize("deg", [0, 50, 70, 90])
def test_expansion_stops_at_a_later_pass(gpu, deg):
    """Response expansion that finds its answer on pass 0 / 1 / 2 / 3 (Mapper.cpp:244-271): kt_select_kernel's
    hand-over to the next pass, and the wider kt_coarse_kernel launches that only the still-empty slots run.
    Precondition: response 0 without expansion and > 0 with it; which window first answers."""
    c = K.expansion()[deg]
    sm = _single(c)
    got = _match_scan(sm, c)
    assert got[2] > 0.0
    _same(got, _oracle_match(("expansion", deg), c))
    assert not sm.grid(0).any()


def test_expansion_mixed_batch(gpu):
    """One batch whose slots end on different passes (aligned, 50, 70 and 90 degrees off: pass 0, 1, 2, 3), twice
    over so that the slots' order differs: every kt_coarse_kernel / kt_select_kernel launch of a pass skips the
    slots that are done or not there yet (S.pass != pass)."""
    ex = K.expansion()
    order = [50, 0, 90, 70, 0, 70, 50, 90]
    c0 = ex[0]
    pool_r = np.concatenate([c0.b_ranges] + [ex[d].q_ranges[None] for d in order])
    pool_p = np.concatenate([c0.b_poses] + [ex[d].q_pose[None] for d in order])
    M = len(order)
    b = K.Batch(pool_r, pool_p, np.arange(1, M + 1, dtype=np.int32), np.arange(M + 1, dtype=np.int32),
                np.zeros(M, np.int32), 1)
    out = _Pooled(b, c0.laser, c0.params).run()
    for i, d in enumerate(order):
        _same_result(out, i, _oracle_match(("expansion", d), ex[d]))


def test_headings_across_pi_and_unnormalised(gpu):
    """Headings 3.04 .. pi .. -3.11 (the mean heading crosses the cut: match 7 returns -3.14127 for a true heading
    of pi) and the same queries 3 turns up / 4 turns down (kt_norm_angle's multi-turn branches)."""
    cases = K.headings()
    sm = _single(cases[0])
    for c in cases:
        _same(_match_scan(sm, c), _oracle_match(c.name, c))


@pytest.mark.parametrize("n", K.SHORT_N)
def test_short_scans(gpu, n):
    """Scans shorter than a wave / a chunk / the block, and one beam off each: kt_prepare_kernel's ragged
    compaction, kt_coarse_kernel's waves without points, and -- the points lie metres apart -- kt_build_kernel's
    fallback from a chunk of 16 to quarters and single points (precondition: a chunk and a quarter of the 64-beam
    scan exceed the 96 x 96-cell LDS tile).  Two matches on one context: slot reuse."""
    cases = K.short(n)
    sm = _single(cases[0])
    for c in cases:
        _same(_match_scan(sm, c), _oracle_match(c.name, c))
        assert not sm.grid(0).any()


@pytest.mark.parametrize("name", ["query_out_of_range", "empty_base", "base_from_behind", "base_partly_outside",
                                  "minimum_range", "all_tie_21", "all_tie_81"])
def test_degenerate_sets(gpu, name):
    """A query without a valid point on a non-empty grid; base scans that are empty, wholly on the wrong side of the
    viewpoint or partly outside the ROI; minimum_range 3.0; and all-tie windows of 441 x 21 and 6561 x 21 poses
    (no base scans, loop parameters): kt_select_kernel's tie compaction across many block rounds."""
    c = K.degenerate()[name]
    sm = _single(c, max_base=3)
    _same(_match_scan(sm, c), _oracle_match(name, c))
    assert not sm.grid(0).any()


# ------------------------------------------------------------------------------------------ run-time knobs
KNOBS = [("SLAM2D_KT_SLOTS", "48"), ("SLAM2D_KT_AG", "3"), ("SLAM2D_KT_AG", "21"), ("SLAM2D_KT_TW", "32"),
         ("SLAM2D_KT_TW", "64"), ("SLAM2D_POISON", "1")]


@pytest.mark.parametrize("knob,value", KNOBS, ids=[f"{k[7:]}={v}" for k, v in KNOBS])
def test_knobs_keep_results(gpu, monkeypatch, knob, value):
    """One setting at a time: SLAM2D_KT_SLOTS=48 (a batch of 130 in chunks of 48, 48, 34), SLAM2D_KT_AG=3 / 21
    (angles per kt_coarse_kernel workgroup), SLAM2D_KT_TW=32 / 64 (32 x 8 and 64 x 4 coarse tiles), SLAM2D_POISON=1
    (every buffer starts as 0xA5 bytes).  A sequential batch of 130 with ragged base counts and a 21 x 21 loop
    batch of 16 must equal the oracle regardless."""
    monkeypatch.setenv(knob, value)
    seq = _Pooled(K.sequential_batch(130, 8), K.laser(), K.params())
    out = seq.run()
    for i in sorted(set(range(0, 130, 9)) | {0, 129}):
        _same_result(out, i, _oracle_match(("seq130", i), seq.case(i)))
    loop = _Pooled(K.loop_batch(16, 6), K.laser(), K.smear_params("loop"))
    out = loop.run(False, False)
    for i in range(16):
        _same_result(out, i, _oracle_match(("loop16", i), loop.case(i, penalize=False, refine=False)))
