"""Stream order across the calls of the three contexts that had no caller-stream test (spa_, kl_, kd_; the ke_, kp_
tests pin it for the others): a call sequence run once on the context's own stream and once with alternate calls on
a torch.cuda.Stream() gives bit-identical results, equal to the plain references the stages' own tests use
(tests/ref/spa2d_ref.py, tests/ref/karto_loop_plain.py); a context closes with its last call still pending; a context
created, closed and created again works as the first (csrc/stage_runtime.h: StreamCall, DeviceBuffers).  And for the
four oldest contexts (hs_, gm_, pl_, ud_), which share that runtime too: what the kernel timer counts per call, on
every launch path, and the same lifetime."""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "ref"))
import karto_loop_plain as LP  # noqa: E402
import karto_loop_ref as KR  # noqa: E402
import spa2d_ref as R  # noqa: E402

from slam2d import karto_edit as kd  # noqa: E402
from slam2d import karto_link as ke  # noqa: E402
from slam2d import karto_loop as kl  # noqa: E402
from slam2d import karto_process as kp  # noqa: E402
from slam2d import spa as sp  # noqa: E402
from slam2d.gmapping import GMappingFleet  # noqa: E402
from slam2d.hector import HectorFleet  # noqa: E402
from slam2d.karto import KtLaser  # noqa: E402
from slam2d.plicp import PLICP  # noqa: E402
from slam2d.undistort import UndistortFleet  # noqa: E402

pytestmark = pytest.mark.gpu

KL_PRM = dict(link_scan_maximum_distance=1.5, loop_search_maximum_distance=4.0, loop_match_minimum_chain_size=3,
              use_scan_barycenter=0)
LASER = dict(minimum_angle=-1.0, angular_resolution=0.25, minimum_range=0.1, range_threshold=4.0, n_readings=8)
PREC = np.array([[120.0, 3.0, -2.0], [3.0, 90.0, 1.5], [-2.0, 1.5, 400.0]])


def dev(a):
    """The bytes of a host array on the device (the copy has finished when this returns)."""
    import torch

    b = np.ascontiguousarray(a).view(np.uint8).reshape(-1)
    t = torch.from_numpy(np.concatenate([b, np.zeros(16, np.uint8)])).cuda()
    torch.cuda.synchronize()
    return t


def streams(alternate):
    """The stream of call 0, 1, 2, ...: the context's own (0), or alternately that and one torch stream."""
    import torch

    other = torch.cuda.Stream() if alternate else None
    return (lambda i: other.cuda_stream if alternate and i % 2 else 0), other


def laser():
    return KtLaser(LASER["minimum_angle"], LASER["angular_resolution"], LASER["minimum_range"], LASER["range_threshold"],
                   LASER["n_readings"], 0)


# ------------------------------------------------------------------------------------------------ spa_
SPA_EXTRA = (0, 100, 102, np.array([0.3, -0.2, 0.1]), PREC)  # graph 0: one more constraint between ids 100 and 102


def spa_cases():
    return [R.case_tiny(4, seed=20), R.case_tiny(4, seed=31)]


def spa_run(alternate):
    cases = spa_cases()
    f = sp.SpaFleet(2, 7, 9)
    for g, c in enumerate(cases):
        f.set_graph(g, c["ids"], c["poses"], c["ends"], c["means"], c["precs"])
    prm = sp.default_params(niter=6)
    row = np.zeros(1, sp.CON_ROW_DTYPE)
    row[0] = (SPA_EXTRA[0], SPA_EXTRA[1], SPA_EXTRA[2], 0, SPA_EXTRA[3], SPA_EXTRA[4].reshape(9))
    d_row, d_added, d_status = dev(row), dev(np.full(1, -7, np.int32)), dev(np.full(1, -7, np.int32))
    on, other = streams(alternate)
    f.compute_device(0, 2, prm, on(0))
    f.edit_constraints_device(1, d_row.data_ptr(), 0, d_added.data_ptr(), d_status.data_ptr(), on(1))
    f.compute_device(0, 2, prm, on(2))
    out = [(f.get_nodes(g), f.stats(g), f.counts(g)) for g in range(2)]  # waits for the last call
    out.append((d_added.cpu().numpy()[:4].view(np.int32)[0], d_status.cpu().numpy()[:4].view(np.int32)[0]))
    f.compute_device(0, 2, prm, on(3))
    f.close()  # with the last compute still pending
    return out


@pytest.fixture(scope="module")
def spa_want():
    """The restatement: compute, add the constraint, compute again; computed once."""
    want = []
    for g, c in enumerate(spa_cases()):
        rg = R.RefGraph()
        for i, p in zip(c["ids"], c["poses"]):
            rg.add_node(i, p)
        for (a, b), m, k in zip(c["ends"], c["means"], c["precs"]):
            assert rg.add_constraint(c["ids"][a], c["ids"][b], m, k)
        prm = dict(c["params"], niter=6)
        rg.compute(prm)
        if g == SPA_EXTRA[0]:
            assert rg.add_constraint(*SPA_EXTRA[1:])
        st = rg.compute(prm)
        want.append((np.asarray(rg.poses), st, (len(rg.ids), len(rg.ends))))
    return want


def test_spa_alternate_streams(gpu, spa_want):
    own, alt = spa_run(False), spa_run(True)
    assert own[2] == alt[2] == (1, 0)  # added, status SPA_OK
    for g in range(2):
        (ids, poses), st, counts = own[g]
        (ids2, poses2), st2, counts2 = alt[g]
        assert ids.tobytes() == ids2.tobytes() and poses.tobytes() == poses2.tobytes() and st == st2
        assert counts == counts2 == spa_want[g][2]
        R.assert_same_result(poses, st, spa_want[g][0], spa_want[g][1], f"graph {g}")


def test_spa_refusal_is_followed_by_a_correct_call_on_another_stream(gpu):
    """The one refusal the suite makes after the call has taken the context (SPA_ERANGE of a device edit on a context
    beyond SPA_EDIT_MAX_NODES): the next call, on another stream, computes what the restatement computes."""
    c = R.case_tiny(4, seed=20)
    f = sp.SpaFleet(1, sp.SPA_EDIT_MAX_NODES + 1, 8)
    f.set_graph(0, c["ids"], c["poses"], c["ends"], c["means"], c["precs"])
    with pytest.raises(sp.Slam2dError) as e:
        f.edit_constraints_device(1, dev(np.zeros(1, sp.CON_ROW_DTYPE)).data_ptr())
    assert e.value.code == sp.SPA_ERANGE
    on, other = streams(True)
    f.compute_device(0, 1, sp.default_params(**c["params"]), on(1))
    (ids, poses), st = f.get_nodes(0), f.stats(0)
    want_poses, want_st = R.compute_case(c)
    R.assert_same_result(poses, st, want_poses, want_st, "after the refusal")
    f.close()


# ------------------------------------------------------------------------------------------------ kl_
def kl_case():
    """8 scans on a circle: neighbours 0.995 apart (within the link distance), a chain of edges 0-1-...-7."""
    ang = 2.0 * np.pi * np.arange(8) / 8.0
    poses = np.stack([1.3 * np.cos(ang), 1.3 * np.sin(ang), ang], axis=1)
    ranges = np.full((8, 8), 2.0) + 0.1 * np.arange(8)[None, :]
    return {"laser": LASER, "params": KL_PRM, "poses": poses, "ranges": ranges,
            "ends": np.array([(i, i + 1) for i in range(7)], np.int32), "queries": np.array([(7, 0, -1, -1), (3, 0, -1, -1)])}


KL_EDGE = (7, 0)  # the device edit: closes the circle


def kl_run(alternate, make=None):
    case = kl_case()
    f = (make or (lambda: kl.LoopSearchFleet(laser(), kl.default_params(**KL_PRM), 1, 11, 9, 3)))()
    f.set_graph(0, 8, case["ends"])
    d_ranges, d_poses = dev(case["ranges"]), dev(case["poses"])
    d_q = dev(kl.queries([(0, *q) for q in case["queries"].tolist()]))
    row = np.zeros(1, kl.EDGE_ROW_DTYPE)
    row[0] = (0, KL_EDGE[0], KL_EDGE[1], 0)
    d_row, d_new, d_status = dev(row), dev(np.full(1, -7, np.int32)), dev(np.full(1, -7, np.int32))
    on, other = streams(alternate)
    f.set_scans_device(0, 0, 8, d_ranges.data_ptr(), d_poses.data_ptr(), on(0))
    f.search_device(2, d_q.data_ptr(), on(1))
    f.edit_edges_device(1, d_row.data_ptr(), d_new.data_ptr(), d_status.data_ptr(), on(2))
    f.search_device(2, d_q.data_ptr(), on(3))
    out = {"slots": [f.get(s) for s in range(2)], "ref": f.get_reference(0, 0, 8), "graph": f.download_graph(0),
           "edit": (d_new.cpu().numpy()[:4].view(np.int32)[0], d_status.cpu().numpy()[:4].view(np.int32)[0]),
           "edit_info": f.edit_info()}
    f.search_device(2, d_q.data_ptr(), on(4))
    f.close()  # with the last search still pending
    return out


def kl_same(a, b):
    for s in range(2):
        for k, v in a["slots"][s].items():
            w = b["slots"][s][k]
            assert (v.tobytes() == w.tobytes()) if isinstance(v, np.ndarray) else v == w, (s, k)
    assert a["ref"].tobytes() == b["ref"].tobytes() and a["edit"] == b["edit"] == (1, 0)
    assert a["edit_info"] == b["edit_info"] == (0, 0)
    for k, v in a["graph"].items():
        w = b["graph"][k]
        assert (v.tobytes() == w.tobytes()) if isinstance(v, np.ndarray) else v == w, k


def kl_check_against_plain(out):
    case = kl_case()
    case["ends"] = np.concatenate([case["ends"], np.array([KL_EDGE], np.int32)])
    assert KR.bits(out["ref"]).tolist() == KR.bits(case["poses"][:, :2]).tolist()  # no barycentre: the pose's position
    assert out["graph"]["ends"].tolist() == case["ends"].tolist()
    for s, q in enumerate(case["queries"]):
        got = out["slots"][s]
        assert got["status"] == kl.KL_OK and got["n_scans"] == 8
        KR.assert_same_search(got, LP.search_case(case, q), f"query {q.tolist()}")


def test_kl_alternate_streams(gpu):
    own, alt = kl_run(False), kl_run(True)
    kl_same(own, alt)
    kl_check_against_plain(own)
    # the edit changed the answer: scan 0 is linked to scan 7 now
    assert 0 in own["slots"][0]["near_link"].tolist()


# ------------------------------------------------------------------------------------------------ kd_
def kd_run(alternate):
    G = 3
    fd = kl.LoopSearchFleet(laser(), kl.default_params(**KL_PRM), G, 6, 8, G)
    sd = sp.SpaFleet(G, 6, 8)
    for g in range(G):  # every graph has scans 0 and 1 already
        for s in range(2):
            assert fd.add_vertex(g) == s
            sd.add_node(g, s, [0.4 * s, 0.1 * g, 0.0])
    edits = kd.GraphEdits(5)
    rec = np.zeros(3, kp.INTAKE_DTYPE)  # graph 0 and 2 accept scan 2; graph 1 does not accept
    for i, accepted in enumerate((1, 0, 1)):
        rec[i]["accepted"], rec[i]["scan"], rec[i]["corrected"] = accepted, 2, [0.8, 0.1 * i, 0.02]
    K = 2
    jobs, links = np.zeros(2, ke.JOB_OUT_DTYPE), np.zeros((2, K), ke.LINK_DTYPE)
    plan = [(0, [(2, 1), (2, 0)]), (2, [(2, 1), (1, 2)])]  # job, graph: two new edges; a new edge and its reverse
    for j, (graph, recs) in enumerate(plan):
        jobs[j]["status"], jobs[j]["n_links"], jobs[j]["graph"] = ke.KE_OK, len(recs), graph
        for r, (a, b) in enumerate(recs):
            links[j, r]["from"], links[j, r]["to"] = a, b
            links[j, r]["diff"], links[j, r]["precision"] = [0.4, 0.01 * j, 0.001 * r], (PREC + r * np.eye(3)).reshape(9)
    d_rec, d_jobs, d_links = dev(rec), dev(jobs), dev(links)
    on, other = streams(alternate)
    edits.commit_vertices_device(d_rec.data_ptr(), 0, 3, fd, sd, on(0))
    edits.commit_edges_device(d_jobs.data_ptr(), d_links.data_ptr(), K, 0, 2, fd, sd, on(1))
    out = {"info": edits.info(), "kl": [fd.download_graph(g) for g in range(G)],
           "spa": [sd.download_graph(g) for g in range(G)], "kl_info": fd.edit_info(), "spa_info": sd.edit_info()}
    edits.commit_edges_device(d_jobs.data_ptr(), d_links.data_ptr(), K, 0, 2, fd, sd, on(2))
    edits.close()  # with the last commit still pending
    fd.close()
    sd.close()
    out["plan"], out["links"] = plan, links
    return out


def test_kd_alternate_streams(gpu):
    own, alt = kd_run(False), kd_run(True)
    assert own["info"] == alt["info"] == (2, 4, 0)  # vertices, new edges, refused rows
    assert own["kl_info"] == alt["kl_info"] == (0, 0) and own["spa_info"] == alt["spa_info"] == (0, 0)
    for key in ("kl", "spa"):
        for g in range(3):
            for k, v in own[key][g].items():
                w = alt[key][g][k]
                assert (v.tobytes() == w.tobytes()) if isinstance(v, np.ndarray) else v == w, (key, g, k)
    # the plain graph the same AddVertex / AddEdge calls build
    for g, n_scans, calls in ((0, 3, own["plan"][0][1]), (1, 2, []), (2, 3, own["plan"][1][1])):
        plain = LP.Graph()
        for _ in range(n_scans):
            plain.add_vertex()
        assert [bool(plain.add_edge(s, t)[1]) for s, t in calls] == [True] * len(calls)
        d = own["kl"][g]
        assert d["n_scans"] == n_scans and d["ends"].tolist() == [list(c) for c in calls]
        got = [d["adj"][d["adj_off"][v]:d["adj_off"][v + 1], 0].tolist() for v in range(n_scans)]
        assert got == [[a.obj for a in v.adjacent()] for v in plain.vertices], g
        s_ = own["spa"][g]
        assert s_["n_nodes"] == n_scans and s_["ends"].tolist() == [list(c) for c in calls]
    for j, g in ((0, 0), (1, 2)):
        s_ = own["spa"][g]
        assert s_["means"].tobytes() == own["links"][j]["diff"].tobytes()
        assert s_["precs"].tobytes() == own["links"][j]["precision"].tobytes()


# ------------------------------------------------------------------------------------------------ rebuild
def test_context_created_closed_and_created_again(gpu):
    """close() frees every buffer the context allocated: the same context can be made again and answers the same."""
    first = kl_run(False)
    made = []

    def make():
        f = kl.LoopSearchFleet(laser(), kl.default_params(**KL_PRM), 1, 11, 9, 3)
        f.close()
        assert not f.h
        f.close()  # closing twice is harmless
        made.append(kl.LoopSearchFleet(laser(), kl.default_params(**KL_PRM), 1, 11, 9, 3))
        return made[0]

    again = kl_run(False, make)
    kl_same(first, again)
    kl_check_against_plain(again)
    for cls, args in ((sp.SpaFleet, (2, 7, 9)), (kd.GraphEdits, (5,)), (ke.LinkStage, (None, 8, 4, 2, 4)),
                      (kp.ProcessStage, (None, 2, 8, 6))):
        a = cls(*args)
        a.close()
        b = cls(*args)
        assert b.h
        b.close()


# ------------------------------------------------------------------------------------------------ hs_
HS_KNOBS = ("SLAM2D_UPDATE", "SLAM2D_UPD_KERNEL", "SLAM2D_PARTS", "SLAM2D_PIPELINE", "SLAM2D_UPD_RAYS_LDS")
HS_N = 3  # steps


def hs_fleet(streams=2, size=64, levels=2, points=32):
    f = HectorFleet(streams, 0.05, size, (0.5, 0.5), levels, max_points=points)
    f.set_thresholds(-1.0, -1.0)  # every step updates the maps
    return f


def hs_scan(streams, points, radius):
    """A ring of end points around every stream's origin, in map scale (cells of level 0), on the device."""
    import torch

    a = 2.0 * np.pi * np.arange(points) / points
    xy = np.stack([radius * np.cos(a), radius * np.sin(a)], axis=1).astype(np.float32)
    d_xy = torch.from_numpy(np.tile(xy, (streams, 1, 1))).cuda()
    d_n = torch.full((streams,), points, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    return xy, d_xy, d_n


def hs_steps(f, streams, points, radius, n=HS_N):
    _, d_xy, d_n = hs_scan(streams, points, radius)
    for _ in range(n):
        f.step_device(d_xy.data_ptr(), points, d_n.data_ptr())
    return f.poses()[0]  # waits for the device


def hs_counts(times):
    assert list(times) == ["match", "bin", "update"]
    assert all((ms > 0.0) == (n > 0) for ms, n in times.values()), times  # every counted launch took time
    return tuple(n for _, n in times.values())


@pytest.fixture
def hs_env(monkeypatch):
    for knob in HS_KNOBS:
        monkeypatch.delenv(knob, raising=False)
    return monkeypatch


def test_hs_launch_counts_default_path(gpu, hs_env):
    f = hs_fleet()
    hs_steps(f, 2, 32, 10.0)  # timing is off at first: nothing is counted
    assert hs_counts(f.kernel_times(reset=False)) == (0, 0, 0)
    f.set_timing(True)
    hs_steps(f, 2, 32, 10.0)
    assert hs_counts(f.kernel_times(reset=False)) == (HS_N, 0, HS_N)
    assert hs_counts(f.kernel_times(reset=True)) == (HS_N, 0, HS_N)  # reset returns the counts ...
    assert hs_counts(f.kernel_times()) == (0, 0, 0)                  # ... and the next read is all zero
    f.set_timing(False)
    hs_steps(f, 2, 32, 10.0)
    assert hs_counts(f.kernel_times()) == (0, 0, 0)  # timing off: the counts do not move
    f.close()


def test_hs_launch_counts_binned_update(gpu, hs_env):
    hs_env.setenv("SLAM2D_UPDATE", "binned")
    f = hs_fleet()
    f.set_timing(True)
    hs_steps(f, 2, 32, 10.0)
    assert hs_counts(f.kernel_times()) == (HS_N, HS_N, HS_N)
    f.close()


def test_hs_launch_counts_match_only(gpu, hs_env):
    f = hs_fleet()
    xy, _, _ = hs_scan(1, 32, 10.0)
    f.set_timing(True)
    f.match(0, xy, np.zeros(3, np.float32))
    assert hs_counts(f.kernel_times()) == (1, 0, 0)
    f.close()


def test_hs_launch_counts_part_streams(gpu, hs_env):
    """128 streams in two parts on their own HIP streams: the timer's one current pair is walked across them."""
    hs_env.setenv("SLAM2D_PARTS", "2")
    f = hs_fleet(128, 32, 1, 16)
    f.set_timing(True)
    hs_steps(f, 128, 16, 5.0)
    assert hs_counts(f.kernel_times()) == (2 * HS_N, 0, 2 * HS_N)
    f.close()


# ------------------------------------------------------------------------------------------------ gm_, pl_
GM_MAP = dict(xmin=-1.6, ymin=-1.6, xmax=1.6, ymax=1.6, delta=0.05, max_range=3.0, max_urange=2.5)  # 64 x 64 cells


def gm_run(n_calls, timing=True):
    """4 particles, 16 beams, n_calls scans and one empty launch: (scores, (ms, launches))."""
    import torch

    f = GMappingFleet(4, max_beams=16, **GM_MAP)
    assert f.size == (64, 64)
    f.set_beams(2.0 * np.pi * np.arange(16) / 16)
    f.set_timing(timing)
    d_poses = torch.from_numpy(GMappingFleet.poses4(np.zeros((4, 3)) + 0.02 * np.arange(4)[:, None])).cuda()
    d_ranges = torch.full((16,), 1.0, dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    for _ in range(n_calls):
        f.compute_device(d_poses.data_ptr(), d_ranges.data_ptr(), 16)
    f.compute_device(d_poses.data_ptr(), d_ranges.data_ptr(), 16, count=0)  # launches nothing
    out = f.scores()[0], f.kernel_times()
    assert f.kernel_times() == (0.0, 0)  # reset is the default
    f.close()
    return out


def test_gm_launch_counts(gpu):
    scores, (ms, launches) = gm_run(3)
    assert launches == 3 and ms > 0.0  # one count per call: the score and the compute kernel are one span
    assert gm_run(3, timing=False)[1] == (0.0, 0)


def pl_run(n_calls, timing=True):
    """2 pairs of 64 rays, n_calls batches and one empty batch: (results' bytes, (ms, launches))."""
    import torch

    n = 64
    ang = -1.0 + 2.0 * np.arange(n) / n
    scan = np.stack([2.0 + 0.3 * np.cos(3.0 * ang), 2.5 + 0.2 * np.sin(2.0 * ang)])
    d_ref, d_sens = torch.from_numpy(scan).cuda(), torch.from_numpy(scan + 0.01).cuda()
    d_guess = torch.zeros((2, 3), dtype=torch.float64, device="cuda")
    d_out = torch.zeros((2, 48), dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    f = PLICP(2, n)
    f.set_timing(timing)
    args = (n, ang[0], 2.0 / n, d_ref.data_ptr(), d_sens.data_ptr(), d_guess.data_ptr(), d_out.data_ptr())
    for _ in range(n_calls):
        f.icp_batch_device(2, *args)
    f.icp_batch_device(0, *args)  # launches nothing
    times = f.kernel_times()  # waits for the device
    out = d_out.cpu().numpy().tobytes(), times
    assert f.kernel_times() == (0.0, 0)
    f.close()
    return out


def test_pl_launch_counts(gpu):
    _, (ms, launches) = pl_run(3)
    assert launches == 3 and ms > 0.0  # one count per batch call
    assert pl_run(3, timing=False)[1] == (0.0, 0)


# ------------------------------------------------------------------------------------------------ lifetime
def closed_and_made_again(make):
    """close() frees what the context allocated: the same context can be made again; closing twice is harmless."""
    a = make()
    a.close()
    assert not a.h
    a.close()
    b = make()
    assert b.h
    return b


def test_oldest_contexts_created_closed_and_created_again(gpu, hs_env):
    first = hs_fleet()
    want = hs_steps(first, 2, 32, 10.0)
    first.close()
    again = closed_and_made_again(hs_fleet)
    assert hs_steps(again, 2, 32, 10.0).tobytes() == want.tobytes()
    again.close()
    again.close()
    assert gm_run(2)[0].tobytes() == gm_run(2)[0].tobytes()  # each run makes and closes its own context
    closed_and_made_again(lambda: GMappingFleet(4, max_beams=16, **GM_MAP)).close()
    assert pl_run(1)[0] == pl_run(1)[0]
    closed_and_made_again(lambda: PLICP(2, 64)).close()
    ud = closed_and_made_again(lambda: UndistortFleet(2, 16, 8))
    ud.set_scan_geometry(-1.0, 0.125, 0.1, 10.0)
    ud.close()
    ud.close()
