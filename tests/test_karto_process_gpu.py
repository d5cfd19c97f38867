"""The Karto scan-intake stage on the GPU (include/slam2d/karto_process.h) against the CPU restatement
tests/ref/karto_process_ref.c.  Bar: bit-exact -- every record, compacted array, count, pool row, advance record and
graph state byte for byte (but for the sign and payload of NaNs, karto_process_ref.canonical_nans), and every byte the
calls must not write still poison.  No tolerance appears anywhere."""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "ref"))
import karto_link_plain as LKP  # noqa: E402
import karto_link_ref as LKR  # noqa: E402
import karto_loop_plain as LP  # noqa: E402
import karto_process_cases as K  # noqa: E402
import karto_process_plain as P  # noqa: E402
import karto_process_ref as R  # noqa: E402
import make_karto_process_golden as G  # noqa: E402
import spa2d_ref as SR  # noqa: E402

from slam2d import karto_link as ke  # noqa: E402
from slam2d import karto_loop as kl  # noqa: E402
from slam2d import karto_process as kp  # noqa: E402
from slam2d.karto import KtLaser, ScanMatcher  # noqa: E402
from slam2d.spa import SpaFleet  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture
def poison(gpu, monkeypatch):
    """SLAM2D_POISON=1: a context's record rows start as 0xA5 bytes, like the restatement's unwritten rows."""
    monkeypatch.setenv("SLAM2D_POISON", "1")
    return True


def dev(a):
    """The bytes of a host array on the device (spare bytes, so that an empty array still has an address)."""
    import torch

    b = np.ascontiguousarray(a).view(np.uint8).reshape(-1)
    return torch.from_numpy(np.concatenate([b, np.zeros(8, np.uint8)])).cuda()


def host(t, dtype, shape):
    n = int(np.prod(shape)) * np.dtype(dtype).itemsize
    return t.cpu().numpy()[:n].copy().view(dtype).reshape(shape)


def sync():
    import torch

    torch.cuda.synchronize()


OUT_TYPES = dict(query=np.int32, base_begin=np.int32, base_index=np.int32, n_seq=np.int32, jobs=R.JOB, queries=R.QUERY,
                 n_jobs=np.int32, items=R.ITEM, pool_ranges=np.float64, pool_poses=np.float64)


class Gpu:
    """karto_process_cases.step's three functions on the device: one ProcessStage per world, seeded with the world's
    graph states; every output starts as the restatement's does (poison, or the world's pools)."""

    def __init__(self, stream=0, calls=1):
        self.st, self.stream, self.calls = None, stream, calls

    def close(self):
        if self.st is not None:
            self.st.close()
            self.st = None

    def stage(self, w):
        self.close()
        st = kp.ProcessStage(kp.default_params(**w["params"]), len(w["states"]), w["n_readings"], w["max_scans"],
                             w["pool_offset"])
        for g, s in enumerate(w["states"]):
            if s["n_scans"]:
                st.set_state(g, s["n_scans"], s["run_begin"], s["run_length"], s["last_time"], s["last_odom"])
        self.st = st
        return st

    def intake(self, w):
        st = self.stage(w)
        e = R.empty_outputs(w)
        self.count, self.pool_scans = len(w["cand"]), len(e["pool_poses"])
        self.d = {k: dev(e[k]) for k in OUT_TYPES}
        d_cand, d_rows = dev(w["cand"]), dev(w["ranges_f32"])
        sync()
        d = self.d
        for _ in range(self.calls):
            st.intake_device(int(w.get("g_first", 0)), self.count, d_cand.data_ptr(), d_rows.data_ptr(), len(w["ranges_f32"]),
                             d["pool_ranges"].data_ptr(), d["pool_poses"].data_ptr(), self.pool_scans, d["query"].data_ptr(),
                             d["base_begin"].data_ptr(), d["base_index"].data_ptr(), self.count * R.window_max(w),
                             d["n_seq"].data_ptr(), d["jobs"].data_ptr(), d["queries"].data_ptr(), d["n_jobs"].data_ptr(),
                             d["items"].data_ptr(), self.stream)
        rec, _ = st.get_intake(0, self.count)
        sync()
        o = {k: host(d[k], t, e[k].shape) for k, t in OUT_TYPES.items()}
        o["rec"] = rec
        return o

    def apply(self, w, rec, seq, pool_poses):
        d_seq = dev(seq)
        self.d["pool_poses"] = dev(pool_poses)
        sync()
        self.st.apply_match_device(d_seq.data_ptr() if len(seq) else 0, len(seq), self.d["pool_poses"].data_ptr(),
                                   self.pool_scans, self.stream)
        rec, _ = self.st.get_intake(0, self.count)
        sync()
        return rec, host(self.d["pool_poses"], np.float64, np.shape(pool_poses))

    def advance(self, w, rec, pool_poses, states=None):
        d_pool = dev(pool_poses)
        sync()
        self.st.advance_device(d_pool.data_ptr(), self.pool_scans, self.stream)
        _, adv = self.st.get_intake(0, self.count)
        states = np.array([self.st.get_state(g) for g in range(len(w["states"]))], R.STATE)
        return adv, states


@pytest.fixture
def gpu_impl(poison):
    g = Gpu()
    yield g
    g.close()


@pytest.fixture(scope="module")
def restated():
    return G.rounds(R)


# ------------------------------------------------------------------------------------ 1. directed cases and the golden
@pytest.mark.parametrize("name", list(K.directed_worlds()))
def test_directed_case(gpu_impl, restated, name):
    got = K.step(gpu_impl, K.directed_worlds()[name])
    K.assert_same_step(got, restated[name], name)


def test_moved_pose_sequence_and_golden(gpu_impl, restated):
    """Two rounds on one context's worth of state, the optimiser moving the last scan in between; the expected records
    come from the fixture the plain transcription wrote: the GPU equals them directly."""
    golden = G.load()
    w, edit, cands = K.moved_sequence()
    a = K.step(gpu_impl, w, edit)
    K.assert_same_step(a, golden["moved_1"], "first round")
    b = K.step(gpu_impl, K.next_world(w, a, cands))
    K.assert_same_step(b, golden["moved_2"], "second round")
    for name in ("gate", "carry", "trim_69_of_70"):
        K.assert_same_step(K.step(gpu_impl, K.directed_worlds()[name]), golden[name], f"golden {name}")


def test_window_longer_than_one_ballot(gpu_impl, restated):
    """70 running scans: the trim takes two rounds of 64 fronts, by distance (69 removed) and by size (one removed)."""
    for name, want in (("69_of_70", (69, 2)), ("one_of_70_by_size", (1, 70)), ("70_kept", (0, 70))):
        w = K.trim_cases()[name][0]
        got = K.step(gpu_impl, w)
        assert (int(got["adv"][0]["run_begin"]), int(got["adv"][0]["run_length"])) == want, name
        before = int(w["states"][0]["run_length"])  # the sequential match is over the whole window before the scan
        assert before >= 69 and got["intake"]["base_index"][:before].tolist() == list(range(before))
        K.assert_same_step(got, restated[f"trim_{name}"], name)


# ------------------------------------------------------------------------------------ 2. launch shapes
@pytest.mark.parametrize("n_graphs", [1, 5, 257])
@pytest.mark.parametrize("n_readings,inverted", [(8, 0), (67, 1)])
def test_fleet_shapes(gpu_impl, n_graphs, n_readings, inverted):
    """One graph; one past a four-wave workgroup; one past a 256-wide prefix block.  67 readings: a tail past one wave,
    read backwards."""
    w = K.fleet_world(n_graphs, n_readings, 20 + n_graphs, inverted)
    want = K.step(R, w)
    if n_graphs == 257:  # absent, rejected, first and later candidates are all there
        rec, present = want["rec"], w["cand"]["row"] >= 0
        assert (~present).any() and (present & (rec["accepted"] == 0)).any()
        assert ((rec["accepted"] == 1) & (rec["prev"] < 0)).any() and ((rec["accepted"] == 1) & (rec["prev"] >= 0)).any()
        assert (rec["match_status"] == R.KT_ERANGE).any() and int(want["intake"]["n_jobs"][0]) > 64
    K.assert_same_step(K.step(gpu_impl, w), want, f"{n_graphs} graphs of {n_readings} readings")


def test_4096_readings(gpu_impl):
    w = K.fleet_world(3, 4096, 7, inverted=1, max_scans=3)
    want = K.step(R, w)
    assert want["rec"]["accepted"].any()
    K.assert_same_step(K.step(gpu_impl, w), want, "4096 readings")


def test_partial_call_leaves_the_other_graphs(gpu_impl):
    """g_first > 0 and count < n_graphs: records past the count stay poison, the other graphs' states stay."""
    w = K.fleet_world(9, 8, 31)
    w["g_first"], w["cand"] = 2, w["cand"][2:7].copy()
    want = K.step(R, w)
    got = K.step(gpu_impl, w)
    K.assert_same_step(got, want, "graphs 2 .. 6 of 9")
    rec, adv = gpu_impl.st.get_intake(0, 9)
    assert rec[5:].tobytes() == R.poisoned(4, R.INTAKE).tobytes() and adv[5:].tobytes() == R.poisoned(4, R.ADVANCED).tobytes()


def test_intake_twice_is_idempotent(poison):
    g = Gpu(calls=2)
    for w in (K.case_gate(), K.fleet_world(257, 8, 5)):
        K.assert_same_step(K.step(g, w), K.step(R, w), "intake called twice")
    g.close()


# ------------------------------------------------------------------------------------ 3. create, state, bind_near, commit
def test_create_refusals_and_state(gpu):
    from slam2d import Slam2dError

    for params, nr, ms in K.refused_creates():
        with pytest.raises(Slam2dError) as e:
            kp.ProcessStage(kp.default_params(**params), 2, nr, ms)
        assert e.value.code == kp.KP_EINVAL
    for params, nr, ms in K.accepted_creates()[2:]:
        kp.ProcessStage(kp.default_params(**params), 2, nr, ms).close()
    st = kp.ProcessStage(kp.default_params(scan_buffer_size=3), 3, 8, 16)
    assert st.get_state(1).tobytes() == R.state().tobytes()
    st.set_state(1, 5, 2, 3, 9.5, (1.0, 2.0, 3.0))
    assert st.get_state(1).tobytes() == R.state(5, 2, 3, 9.5, (1.0, 2.0, 3.0)).tobytes()
    assert st.get_state(0).tobytes() == R.state().tobytes() == st.get_state(2).tobytes()
    for bad in ((5, 1, 4), (5, 2, 2), (0, 0, 1), (17, 14, 3)):
        with pytest.raises(Slam2dError):
            st.set_state(1, *bad, 0.0, (0.0, 0.0, 0.0))
    with pytest.raises(Slam2dError):
        st.set_state(3, 1, 0, 1, 0.0, (0.0, 0.0, 0.0))
    st.clear_graph(1)
    assert st.get_state(1).tobytes() == R.state().tobytes()
    # a base list that could be truncated is refused before anything runs
    with pytest.raises(Slam2dError) as e:
        st.intake_device(0, 3, 1, 1, 1, 1, 1, 48, 1, 1, 1, 8, 1, 0, 0, 1, 0)
    assert e.value.code == kp.KP_EINVAL and "base_capacity" in str(e.value)
    st.close()


@pytest.mark.parametrize("n_jobs", [1, 5, 70])
def test_bind_near(poison, n_jobs):
    """The job rows of an intake get their ranges of a near batch ordered by slot; rows past the job count stay."""
    rng = np.random.default_rng(n_jobs)
    w = K.build_world([dict() for _ in range(n_jobs + 2)], [(None, 1.0, (0.0, 0.0, 0.0))] * n_jobs + [(-1, 0.0, (0.0, 0.0, 0.0))] * 2,
                      n_readings=2, max_scans=2)
    g = Gpu()
    o = g.intake(w)
    assert int(o["n_jobs"][0]) == n_jobs
    slots = np.sort(rng.integers(0, n_jobs, 3 * n_jobs))
    src = np.zeros(len(slots) + 3, R.SOURCE)
    src["slot"][:len(slots)] = slots
    src["slot"][len(slots):] = 0  # past *d_n_matches: not read as matches
    d_src, d_n = dev(src), dev(np.array([len(slots)], np.int32))
    sync()
    g.st.bind_near_device(g.d["jobs"].data_ptr(), d_src.data_ptr(), d_n.data_ptr(), len(src))
    sync()
    got = host(g.d["jobs"], R.JOB, n_jobs + 2)
    want = R.bind_near(o["jobs"], n_jobs, src, len(slots))
    R.assert_same_records(got, want, "bound jobs")
    R.assert_same_records(want[:n_jobs], P.bind_near(o["jobs"], n_jobs, src, len(slots))[:n_jobs], "against the transcription")
    assert int(got["near_count"][:n_jobs].sum()) == len(slots)
    g.close()


# ------------------------------------------------------------------------------------ 4. the consumer contract
LASER = dict(minimum_angle=-1.0, angular_resolution=0.25, minimum_range=0.1, range_threshold=4.0, n_readings=8)


def laser():
    return KtLaser(*[LASER[k] for k in ("minimum_angle", "angular_resolution", "minimum_range", "range_threshold", "n_readings")], 0)


def test_batch_arrays_feed_the_matcher_unchanged(gpu):
    """Two graphs with three running scans each: kt_match_batch_device on the arrays intake wrote equals, bit for bit,
    the same matches on arrays built by the host."""
    rng = np.random.default_rng(2)
    graphs = [dict(poses=[(0.05 * k + 0.3 * g, 0.02 * k, 0.01 * k) for k in range(3)]) for g in range(2)]
    cands = [(None, 4000.0, (0.17 + 0.3 * g, 0.05, 0.03)) for g in range(2)]
    w = K.build_world(graphs, cands, n_readings=8, max_scans=6, seed=9)
    P_ = len(w["pool_poses"])
    w["pool_poses"] = np.where(np.isin(np.arange(P_), [0, 1, 2, 7, 8, 9])[:, None], w["pool_poses"], 0.0)
    room = rng.uniform(1.0, 3.0, 8).astype(np.float32)  # the robots barely move: every scan sees the same ranges
    w["pool_ranges"] = np.tile(room.astype(np.float64), (P_, 1))
    w["ranges_f32"] = np.tile(room, (3, 1))
    g = Gpu()
    o = g.intake(w)
    assert int(o["n_seq"][0]) == 2 and o["base_begin"].tolist() == [0, 3, 6]
    km = ScanMatcher(laser(), None, 2, P_, 8)
    km.set_scans_device(0, P_, g.d["pool_ranges"].data_ptr(), g.d["pool_poses"].data_ptr())
    d_a, d_b = dev(R.poisoned(2, R.KT_RESULT)), dev(R.poisoned(2, R.KT_RESULT))
    sync()
    km.match_batch_device(2, g.d["query"].data_ptr(), g.d["base_begin"].data_ptr(), g.d["base_index"].data_ptr(), d_a.data_ptr())
    sync()
    off = w["pool_offset"]
    h_q, h_bb = dev(np.array([off[0] + 3, off[1] + 3], np.int32)), dev(np.array([0, 3, 6], np.int32))
    h_bi = dev(np.array([off[0], off[0] + 1, off[0] + 2, off[1], off[1] + 1, off[1] + 2], np.int32))
    sync()
    km.match_batch_device(2, h_q.data_ptr(), h_bb.data_ptr(), h_bi.data_ptr(), d_b.data_ptr())
    sync()
    a, b = host(d_a, R.KT_RESULT, 2), host(d_b, R.KT_RESULT, 2)
    assert a.tobytes() == b.tobytes() and (a["status"] == 0).all()
    km.close()
    g.close()


# ------------------------------------------------------------------------------------ 5. a short fleet replay
REPLAY_PARAMS = dict(scan_buffer_size=4, scan_buffer_maximum_scan_distance=1.0)
KL_PRM = dict(link_scan_maximum_distance=1.5, loop_search_maximum_distance=4.0, loop_match_minimum_chain_size=3,
              use_scan_barycenter=0)
# per round and graph: the step along the heading since the previous candidate, or None (no scan this round)
STEPS = [[0.0, 0.3, 0.05, 0.3, 0.3, 0.02, 0.3, 0.75, 0.3, 0.01, 0.3, 0.3, 0.3, 0.04],
         [0.0, 0.25, None, 0.03, 0.4, 0.4, 0.02, 0.02, 0.4, 0.9, None, 0.3, 0.3, 0.3]]
MOVE_AFTER_ROUND = 6  # the optimiser moves every graph's last scan after this round's advance


def replay_candidates(k):
    cands = []
    for g in range(2):
        s = STEPS[g][k]
        if s is None:
            cands.append((-1, 0.0, (0.0, 0.0, 0.0)))
            continue
        d = sum(v for v in STEPS[g][:k + 1] if v is not None)
        cands.append((None, 10.0 * k, (d * np.cos(0.2 + g), d * np.sin(0.2 + g), 0.2 + g + 0.01 * k)))
    return cands


class PlainGraph:
    """One graph's MapperGraph and SPA system by the transcriptions."""

    def __init__(self):
        self.g, self.spa = LP.Graph(), SR.RefGraph()

    def ends(self):
        return [(e.source.obj, e.target.obj) for e in self.g.edges]


def plain_link_round(w, o, rec, pool, seq, graphs):
    """AddVertex / AddNode, the running chain's closest scan, AddEdges and the commit, by the transcriptions: the pool
    poses after AddEdges' pose write."""
    n_jobs, n_seq = int(o["n_jobs"][0]), int(o["n_seq"][0])
    running = np.zeros(n_seq, LKR.CLOSEST)
    for i, r in enumerate(rec):
        if not r["accepted"]:
            continue
        pg = graphs[int(w.get("g_first", 0)) + i]
        assert pg.g.add_vertex() == r["scan"]
        pg.spa.add_node(int(r["scan"]), r["corrected"])
        if r["seq"] >= 0:
            off = int(w["pool_offset"][i])
            ref = [(float(x), float(y)) for x, y in pool[off:off + int(r["scan"]) + 1, :2]]
            chain = list(range(int(r["run_begin"]), int(r["run_begin"]) + int(r["run_length"])))
            closest, linked = LP.link_test(ref, chain, int(r["scan"]), KL_PRM["link_scan_maximum_distance"])
            running[int(r["seq"])] = (closest, linked)
    world = dict(jobs=o["jobs"][:n_jobs], pool_poses=pool, seq=seq[:n_seq], running=running, near=np.zeros(0, LKR.KT_RESULT),
                 near_source=np.zeros(0, LKR.SOURCE), near_chains=np.zeros((0, 0), LKR.NEAR_CHAIN),
                 params=dict(link_match_minimum_response_fine=0.8), max_links=8, flags=LKR.KE_WRITE_POSE)
    links, out, pool2 = LKP.add_edges(world)
    for j in range(n_jobs):
        pg = graphs[int(out[j]["graph"])]
        for l_ in links[j, :int(out[j]["n_links"])]:
            if l_["status"] == LKR.KE_OK and pg.g.add_edge(int(l_["from"]), int(l_["to"]))[1]:
                assert pg.spa.add_constraint(int(l_["from"]), int(l_["to"]), l_["diff"].tolist(), l_["precision"].tolist())
    return running, links, out, pool2


def test_fleet_replay(poison):
    """intake -> synthetic matches -> apply -> kp_commit_vertices -> kl_closest_device -> ke_add_edges_device
    (KE_WRITE_POSE) -> ke_commit -> kp_advance_device for two graphs over 14 rounds, against the transcriptions driving
    karto_link_plain / karto_loop_plain for the same rounds."""
    import torch

    w = K.build_world([dict(), dict()], replay_candidates(0), REPLAY_PARAMS, n_readings=8, max_scans=16, seed=40)
    P_ = len(w["pool_poses"])
    w["pool_poses"], w["pool_ranges"] = np.zeros((P_, 3)), np.full((P_, 8), 5.0)
    w["ranges_f32"] = np.random.default_rng(41).uniform(0.5, 9.0, (2, 8)).astype(np.float32)
    st = kp.ProcessStage(kp.default_params(**w["params"]), 2, 8, 16, w["pool_offset"])
    f = kl.LoopSearchFleet(laser(), kl.default_params(**KL_PRM), 2, 16, 64, 2)
    spa = SpaFleet(2, 16, 64)
    link = ke.LinkStage(ke.default_params(), 8, 2, 8, 1)
    for g in range(2):
        f.set_pool_offset(g, int(w["pool_offset"][g]))
    d_pool, d_ranges = torch.from_numpy(w["pool_poses"].copy()).cuda(), torch.from_numpy(w["pool_ranges"].copy()).cuda()
    d_rows = dev(w["ranges_f32"])
    graphs = [PlainGraph(), PlainGraph()]
    rejected, accepted, by_size, by_distance, moved_rounds = [0, 0], [0, 0], 0, 0, 0
    size = REPLAY_PARAMS["scan_buffer_size"]
    for k in range(len(STEPS[0])):
        # ---- the transcription's round
        o = P.intake(w)
        n_jobs, n_seq = int(o["n_jobs"][0]), int(o["n_seq"][0])
        seq = K.results([o["rec"][i]["sensor"] + [0.01, -0.005, 0.002] for i in range(2) if o["rec"][i]["seq"] >= 0], seed=k)
        rec, pool = P.apply(w, o["rec"], seq, o["pool_poses"])
        running, links, out, pool = plain_link_round(w, o, rec, pool, seq, graphs)
        adv, states = P.advance(w, rec, pool)
        for g in range(2):
            if w["cand"][g]["row"] >= 0:
                accepted[g] += int(rec[g]["accepted"])
                rejected[g] += 1 - int(rec[g]["accepted"])
            if rec[g]["accepted"]:
                removed = int(rec[g]["run_length"]) + 1 - int(adv[g]["run_length"])
                forced = max(0, int(rec[g]["run_length"]) + 1 - size)
                by_size += forced > 0
                by_distance += removed > forced
        # ---- the device's round
        e = R.empty_outputs(w)
        d = {name: dev(e[name]) for name in ("query", "base_begin", "base_index", "n_seq", "jobs", "queries", "n_jobs", "items")}
        d_cand, d_seq, d_running = dev(w["cand"]), dev(seq), dev(R.poisoned(2, LKR.CLOSEST))
        sync()
        st.intake_device(0, 2, d_cand.data_ptr(), d_rows.data_ptr(), 2, d_ranges.data_ptr(), d_pool.data_ptr(), P_,
                         d["query"].data_ptr(), d["base_begin"].data_ptr(), d["base_index"].data_ptr(), 2 * size,
                         d["n_seq"].data_ptr(), d["jobs"].data_ptr(), d["queries"].data_ptr(), d["n_jobs"].data_ptr(),
                         d["items"].data_ptr())
        st.apply_match_device(d_seq.data_ptr() if n_seq else 0, n_seq, d_pool.data_ptr(), P_)
        assert st.commit_vertices(f, spa) == n_jobs
        got_rec, _ = st.get_intake(0, 2)
        R.assert_same_records(got_rec, rec, f"round {k} records")
        for name in ("query", "base_begin", "base_index", "n_seq", "jobs", "queries", "n_jobs", "items"):
            R.assert_same_records(host(d[name], OUT_TYPES[name], e[name].shape), o[name], f"round {k} {name}")
        for g in range(2):
            n = f.counts(g)[0]
            off = int(w["pool_offset"][g])
            if n:
                f.set_scans_device(g, 0, n, d_ranges[off:].data_ptr(), d_pool[off:].data_ptr())
        if n_seq:
            f.closest_device(n_seq, d["items"].data_ptr(), d_running.data_ptr())
        if n_jobs:
            link.add_edges_device(n_jobs, d["jobs"].data_ptr(), d_pool.data_ptr(), P_, d_seq.data_ptr() if n_seq else 0, n_seq,
                                  d_running.data_ptr() if n_seq else 0, n_seq, 0, 0, 0, 0, 0, 0, ke.KE_WRITE_POSE)
            got_links, got_out = link.get_links(0, n_jobs)
            LKR.assert_same_records(got_out, out, f"round {k} AddEdges outputs")
            for j in range(n_jobs):
                LKR.assert_same_records(got_links[j, :out[j]["n_links"]], links[j, :out[j]["n_links"]], f"round {k} links")
            link.commit(f, spa, 0, n_jobs)
        sync()
        if n_seq:
            assert host(d_running, LKR.CLOSEST, n_seq).tobytes() == running.tobytes(), f"round {k} running chain"
        st.advance_device(d_pool.data_ptr(), P_)
        _, got_adv = st.get_intake(0, 2)
        R.assert_same_records(got_adv, adv, f"round {k} advance records")
        R.assert_same_records(np.array([st.get_state(g) for g in range(2)], R.STATE), states, f"round {k} states")
        R.assert_same_records(d_pool.cpu().numpy(), pool, f"round {k} pool poses")
        R.assert_same_records(d_ranges.cpu().numpy(), o["pool_ranges"], f"round {k} pool ranges")
        for g in range(2):
            pg = graphs[g]
            assert f.counts(g) == (len(pg.g.vertices), len(pg.g.edges)) and spa.counts(g) == (len(pg.spa.ids), len(pg.spa.ends))
            ids, poses = spa.get_nodes(g)
            assert ids.tolist() == pg.spa.ids
            R.assert_same_records(poses, np.asarray(pg.spa.poses, np.float64).reshape(-1, 3), f"round {k} node poses of graph {g}")
        # ---- the optimiser moves the last scans between this advance and the next intake
        if k == MOVE_AFTER_ROUND:
            for g in range(2):
                slot = int(w["pool_offset"][g]) + int(states[g]["n_scans"]) - 1
                pool[slot] = pool[slot] + [0.03, -0.02, 0.01]
                moved_rounds += 1
            d_pool = torch.from_numpy(pool.copy()).cuda()
        w = dict(w, states=states, pool_poses=pool, pool_ranges=o["pool_ranges"])
        if k + 1 < len(STEPS[0]):
            nxt = replay_candidates(k + 1)
            rows, r = [], 0
            for row, _, _ in nxt:
                rows.append(row if row is not None else r)
                r += row is None
            w["cand"] = R.candidates(rows, [c[1] for c in nxt], [c[2] for c in nxt])
    # ---- the replay is not vacuous (asserted on the transcription alone)
    assert min(rejected) >= 3 and min(accepted) >= 8, (rejected, accepted)
    assert by_size >= 1 and by_distance >= 1, (by_size, by_distance)
    assert moved_rounds >= 1
    for g in range(2):
        ends = graphs[g].ends()
        assert len(ends) >= accepted[g] - 1 and all(a < b for a, b in ends)
    link.close()
    spa.close()
    f.close()
    st.close()


# ------------------------------------------------------------------------------------ 6. streams and timing
def test_caller_stream_and_timing(poison):
    import torch

    w = K.fleet_world(5, 8, 3)
    want = K.step(R, w)
    s = torch.cuda.Stream()
    g = Gpu(stream=s.cuda_stream)
    with torch.cuda.stream(s):
        st = g.stage(w)
        st.set_timing(True)
        g.stage = lambda _w: st
        got = K.step(g, w)
        s.synchronize()
    K.assert_same_step(got, want, "on a caller's stream")
    times = st.kernel_times(reset=True)
    assert {k: v[1] for k, v in times.items()} == {"kp_intake_kernel": 1, "kp_compact_kernel": 1, "kp_store_kernel": 1,
                                                   "kp_apply_kernel": 1, "kp_bind_near_kernel": 0, "kp_advance_kernel": 1}
    assert all(v[0] > 0.0 for k, v in times.items() if k != "kp_bind_near_kernel")
    assert all(v == (0.0, 0) for v in st.kernel_times().values())
    st.close()
