"""Karto correlative matcher without a GPU: the CPU restatement (oracle/karto_oracle.c) behaves like
open_karto's ScanMatcher on the reference's own parameters, and kt_create validates parameters
before touching a device.  open_karto needs boost (absent): parity against it is unpinned."""
import ctypes as C
import math

import numpy as np
import pytest

import oracle as O
from slam2d import synth

D = math.pi / 180.0


def laser(thr=12.0):
    return O.KtLaser(float(synth.ANGLE_MIN), float(synth.ANGLE_INC), 0.1, thr, synth.N_BEAMS, 0)


def params(loop=False, expansion=0):
    # Mapper::InitializeParameters (Mapper.cpp:1569-1660)
    if loop:
        return O.KtParams(8.0, 0.05, 0.03, 0.3 ** 2, (20 * D) ** 2, 0.2 * D, 20 * D, 2 * D, 0.9, 0.5, expansion, 0)
    return O.KtParams(0.3, 0.01, 0.03, 0.3 ** 2, (20 * D) ** 2, 0.2 * D, 20 * D, 2 * D, 0.9, 0.5, expansion, 0)


def test_grid_geometry_matches_create():
    """ScanMatcher::Create (Mapper.cpp:150-160) + CorrelationGrid border / WidthStep (Mapper.h:925,
    Karto.h:4442): 0.3 m / 0.01 m, range 12 m -> side 31, grid 31 + 2*1200, border Round(6)+1."""
    g = O.karto_grid_info(params(), laser())
    assert (g["side"], g["grid_size"], g["border"], g["width"], g["ws"]) == (31, 2431, 7, 2445, 2448)
    assert (g["half"], g["ksize"]) == (6, 13)
    lg = O.karto_grid_info(params(loop=True), laser())
    assert (lg["side"], lg["grid_size"], lg["border"], lg["ksize"]) == (161, 641, 2, 3)


def test_smear_kernel_values():
    """CalculateKernel (Mapper.h:1046-1086): Round(100 exp(-d^2 / (2 sigma^2))) on the 13x13 support."""
    k = np.zeros(169, np.uint8)
    assert O.karto_lib().ko_kernel(params(), laser(), O._fp(k), 169) == 169
    k = k.reshape(13, 13)
    i = np.arange(-6, 7)
    d2 = (i[:, None] * 0.01) ** 2 + (i[None, :] * 0.01) ** 2
    expect = np.floor(np.exp(-0.5 * d2 / 0.03 ** 2) * 100 + 0.5)
    assert np.array_equal(k, expect.astype(np.uint8))
    assert k[6, 6] == 100 and (k[np.arange(13) != 6].max() < 100)


def test_sequential_match_recovers_pose():
    R, T, Q = synth.karto_sequential(3, 10, seed=1)
    for i in range(10, 13):
        m, c, r = O.karto_match(laser(), params(), R[i], Q[i], R[i - 10:i], T[i - 10:i])
        assert np.abs(m[:2] - T[i][:2]).max() < 0.02
        assert abs(m[2] - T[i][2]) < 0.01
        assert 0.5 < r <= 1.0
        assert np.allclose(c, c.T) and np.all(np.diag(c) > 0)


def test_loop_match_recovers_drift():
    QR, qp, qt, CR, CP = synth.karto_loop(2, seed=2)
    for i in range(2):
        m, c, r = O.karto_match(laser(), params(loop=True), QR[i], qp[i], CR[i], CP[i], False, True)
        assert np.abs(m[:2] - qt[i][:2]).max() < 0.06, (m, qt[i])
        assert r > 0.3


def test_empty_grid_averages_whole_window():
    """No base scans: every response is 0, all 16x16x21 poses tie, the mean is the window centre and
    the covariance is MAX_VARIANCE (Mapper.cpp:545-551)."""
    R, T, Q = synth.karto_sequential(1, 1, seed=1)
    m, c, r = O.karto_match(laser(), params(), R[1], Q[1], R[:0], T[:0], True, False)
    assert r == 0.0
    assert abs(m[0] - Q[1][0]) < 1e-9 and abs(m[1] - Q[1][1]) < 1e-9
    assert c[0, 0] == 500.0 and c[1, 1] == 500.0


def test_kt_create_rejects_unsupported_params():
    """kt_create validates like ScanMatcher::Create / CalculateKernel before any device call."""
    from slam2d import karto

    L = karto._lib.lib()
    karto._declare(L)
    lz = karto.laser(synth.N_BEAMS, float(synth.ANGLE_MIN), float(synth.ANGLE_INC), 0.1, 12.0)
    h = C.c_void_p()
    bad = karto.default_params()
    bad.smear_deviation = 10 * bad.resolution  # off-centre kernel value 100 -> order-dependent AddScan
    assert L.kt_create(C.byref(h), C.byref(lz), C.byref(bad), 1, 4, 3) == -1
    assert b"off-centre" in L.kt_last_error()
    bad = karto.default_params()
    bad.smear_deviation = 0.1 * bad.resolution
    assert L.kt_create(C.byref(h), C.byref(lz), C.byref(bad), 1, 4, 3) == -1
    p = karto.default_params()
    assert p.search_size == 0.3 and p.resolution == 0.01 and abs(p.coarse_search_angle_offset - 20 * D) < 1e-15


# ----------------------------------------------------------------------------- sharded window (gloo)
def _window_case():
    lz = laser()
    p = params(loop=True)
    p.search_size = 2.0  # 21 x 21 coarse positions x 21 angles
    QR, qp, _, CR, CP = synth.karto_loop(1, 4, seed=31, perturb=(0.2, 0.2, 0.03))
    resp = O.karto_coarse_responses(lz, p, QR[0], qp[0], CR[0], CP[0], 21, 21, penalize=True)
    return resp


def _window_worker(rank, world, port, out):
    import os
    import torch
    import torch.distributed as dist

    from slam2d import karto

    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    resp = _window_case()
    nA = resp.shape[2]
    mine = resp.copy()
    for a in range(nA):  # what this rank's kt_coarse_kernel leaves: other ranks' angles +0.0
        if not karto.shard_owns_angle(a, rank, world):
            mine[:, :, a] = 0.0
    posmax = mine.max(axis=2)
    best = mine.max()
    x = torch.from_numpy(np.concatenate([[best], posmax.ravel(), mine.ravel()]).view(np.int64).copy())
    karto.allreduce_window(x)
    out[rank] = x.numpy().tobytes()
    dist.barrier()
    dist.destroy_process_group()


@pytest.mark.parametrize("world", [2, 3])
def test_sharded_window_exchange_gloo(world):
    """the exchange step of a Karto window split over ranks by angle (the same
    slam2d.karto.allreduce_window the GPU path calls, here over gloo): after the int64 MAX all-reduce
    every rank holds, bit for bit, the unsharded window's responses, per-position maxima and best --
    the inputs of the tie average and covariance, which then run identically on every rank."""
    import socket

    import torch.multiprocessing as mp

    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    with mp.Manager() as m:
        out = m.dict()
        mp.spawn(_window_worker, args=(world, port, out), nprocs=world, join=True)
        res = dict(out)
    resp = _window_case()
    assert np.all(resp >= 0.0) and resp.max() > 0.0
    want = np.concatenate([[resp.max()], resp.max(axis=2).ravel(), resp.ravel()])
    for r in range(world):
        got = np.frombuffer(res[r], np.float64)
        assert np.array_equal(got.view(np.int64), want.view(np.int64)), r


# ----------------------------------------------------------------------------- path-test preconditions
def test_path_case_preconditions():
    """tests/ref/karto_cases.py builds the inputs of tests/test_karto_paths_gpu.py; each case reaches its kernel
    path only while its generator keeps a property, asserted here with the oracle alone -- a drifting generator
    fails here instead of silently no longer reaching the path."""
    import os
    import sys

    sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "ref"))
    import karto_cases as K

    # smear sizes: every branch of kt_group (ks <= 15 | > 15) and kt_addscans_kernel (<= 13 | 15 | > 15)
    for ks, dev in K.SMEAR.items():
        g = O.karto_grid_info(K.smear_params(ks), K.laser())
        assert (g["ksize"], g["half"]) == (ks, ks // 2), (dev, g)
    assert O.karto_grid_info(K.smear_params("loop"), K.laser())["ksize"] == 3
    assert O.karto_grid_info(K.smear_params(41), K.laser())["half"] > 16  # beyond the 16-cell LDS tile margin

    # ko_count_valid against the plain restatement of FindValidPoints + AddScan's ROI test, on two scans
    far = K.degenerate()["base_partly_outside"]
    per = far.count_valid()
    for b in range(2):
        pts, valid = K.find_valid_points(far.laser, far.b_ranges[b], far.b_poses[b], far.q_pose[:2])
        _, inside = K.roi_cells(far, pts)
        assert per[b] == int((valid & inside).sum()), b
        if b == 1:  # the base scan 15 m away: partly outside the ROI
            assert 0 < per[b] < int(valid.sum())

    # dense scan: kt_coarse_kernel's 16-bit flush (504 points per wave; a wave takes a quarter of the points; the
    # unflushed packed sum of the best pose would pass 65535), kt_prepare_kernel's LDS above 64 KB, kt_fine_kernel's
    # fourth register round, and every base scan within kt_addscans_kernel's item store (not reached here: the
    # grid has more than 2048 tiles, but the bound is what keeps its pass loop advancing)
    dn = K.dense()
    pts, _ = K.find_valid_points(dn.laser, dn.q_ranges, dn.q_pose, dn.q_pose[:2])
    npts = len(pts)
    resp = O.karto_coarse_responses(dn.laser, dn.params, dn.q_ranges, dn.q_pose, dn.b_ranges, dn.b_poses, 16, 21, False)
    assert npts > 2045 and resp.max() * npts * 25 > 65535, (npts, resp.max())
    assert dn.laser.n_readings * 24 > 65536 and npts > 3 * 4 * 256
    assert max(K.footprint_items(dn, b) for b in range(5)) <= K.KT_AS_ITEMS

    # many base scans: more valid points (a lower bound of the footprint items) than one pass of
    # kt_addscans_kernel holds, for every match whose grid is read; no single base scan overflows it
    mb = K.many_base_batch()
    for ks in (13, 41):
        for i in (0, mb.count // 2, mb.count - 1):
            c = mb.case(i, K.laser(), K.smear_params(ks))
            assert int(c.count_valid().sum()) > K.KT_AS_ITEMS, (ks, i)
            if i == 0:
                assert max(K.footprint_items(c, b) for b in range(len(c.b_ranges))) <= K.KT_AS_ITEMS

    # expansion that stops late: nothing inside +-20 degrees for the rotated queries, and the pass that answers
    ex = K.expansion()
    assert ex[0].match()[2] > 0.5
    for deg, zero_at, hit_at in ((50, 20, 40), (70, 40, 60), (90, 60, 80)):  # answered by pass 1, 2, 3
        assert ex[deg].match()[2] > 0.0
        assert ex[deg].with_params("off", use_response_expansion=0).match()[2] == 0.0
        at = lambda a: ex[deg].with_params("a", use_response_expansion=0, coarse_search_angle_offset=a * D).match()[2]
        assert at(zero_at) == 0.0 and at(hit_at) > 0.0, deg

    # headings straddle +-pi; the unnormalised queries are the same headings 3 and 4 turns away
    hd = K.headings()
    hs = np.array([c.q_pose[2] for c in hd if abs(c.q_pose[2]) < 4])
    assert hs.min() < -3.0 and hs.max() > 3.0 and any(c.b_poses[-1, 2] == math.pi for c in hd)
    assert sum(abs(c.q_pose[2]) > 15 for c in hd) == 2 * len(hs)
    assert any(c.match()[0][2] < -3.1 for c in hd if c.b_poses[-1, 2] > 3.1)  # a mean across the cut

    # short scans: some chunk of 16 points and some quarter of 4 do not fit the 96 x 96-cell LDS tile of
    # kt_build_kernel (the quarter and single-point fallbacks)
    c = K.short(64)[0]
    h = O.karto_grid_info(c.params, c.laser)["half"]
    pts, valid = K.find_valid_points(c.laser, c.b_ranges[0], c.b_poses[0], c.q_pose[:2])
    cells, inside = K.roi_cells(c, pts)
    ok = valid & inside

    def misfit(size):
        n = 0
        for k0 in range(0, len(pts), size):
            sel = cells[k0:k0 + size][ok[k0:k0 + size]]
            if len(sel) > 1 and (sel.max(axis=0) - sel.min(axis=0) + 2 * h + 1).max() > 96:
                n += 1
        return n

    assert misfit(16) > 0 and misfit(4) > 0
    assert [len(K.short(n)) for n in K.SHORT_N] == [2] * len(K.SHORT_N)
    assert K.short(1)[0].count_valid().sum() == 0 and K.short(15)[0].count_valid().sum() > 0

    # degenerate sets
    dg = K.degenerate()
    assert not np.any(dg["query_out_of_range"].q_ranges <= 12.0) and dg["query_out_of_range"].count_valid().sum() > 0
    assert dg["query_out_of_range"].match()[2] == 0.0
    assert list(dg["empty_base"].count_valid() > 0) == [True, False, True]
    bh = dg["base_from_behind"]
    assert int(np.sum(bh.b_ranges[0] <= 12.0)) == 62 and list(bh.count_valid() > 0) == [False, True]
    front = K.Case("front", bh.laser, bh.params, bh.q_ranges, bh.b_poses[0], bh.b_ranges, bh.b_poses)
    assert front.count_valid()[0] > 0  # the same patch from its own side is valid
    mr = dg["minimum_range"]
    lo = K.Case("lo", K.laser(), mr.params, mr.q_ranges, mr.q_pose, mr.b_ranges, mr.b_poses)
    assert np.all(mr.count_valid() < lo.count_valid()) and np.all(mr.count_valid() > 0)
    assert np.sum((mr.q_ranges >= 0.1) & (mr.q_ranges < 3.0)) > 0
    for name, ties in (("all_tie_21", 441 * 21), ("all_tie_81", 6561 * 21)):
        c = dg[name]
        assert len(c.b_ranges) == 0 and ties > 1024  # more than one block round of kt_select_kernel
        m, cov, r = c.match()
        assert r == 0.0 and abs(m[0] - c.q_pose[0]) < 1e-9 and abs(m[1] - c.q_pose[1]) < 1e-9
