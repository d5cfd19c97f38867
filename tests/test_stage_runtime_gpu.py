"""Stream order across the calls of the three contexts that had no caller-stream test (spa_, kl_, kd_; the ke_, kp_
tests pin it for the others): a call sequence run once on the context's own stream and once with alternate calls on
a torch.cuda.Stream() gives bit-identical results, equal to the plain references the stages' own tests use
(tests/ref/spa2d_ref.py, tests/ref/karto_loop_plain.py); a context closes with its last call still pending; a context
created, closed and created again works as the first (csrc/stage_runtime.h: StreamCall, DeviceBuffers)."""
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
from slam2d.karto import KtLaser  # noqa: E402

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
