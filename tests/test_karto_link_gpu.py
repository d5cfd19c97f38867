"""The Karto graph-linking stage on the GPU (include/slam2d/karto_link.h) against the CPU restatement
tests/ref/karto_link_ref.c, on synthetic matcher results (the matcher itself is not run here).  Bar: bit-exact --
every record, job output, closure, fine-batch array, tmp row and written pool pose byte for byte, and every byte the
calls must not write still poison.  No tolerance appears anywhere."""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "ref"))
import karto_link_cases as K  # noqa: E402
import karto_link_plain as P  # noqa: E402
import karto_link_ref as R  # noqa: E402
import karto_loop_plain as LP  # noqa: E402
import make_karto_link_golden as G  # noqa: E402
import spa2d_ref as SR  # noqa: E402

from slam2d import karto_link as ke  # noqa: E402
from slam2d import karto_loop as kl  # noqa: E402
from slam2d.karto import KtLaser  # noqa: E402
from slam2d.spa import SpaFleet  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture
def poison(gpu, monkeypatch):
    """SLAM2D_POISON=1: a context's link rows start as 0xA5 bytes, like the restatement's unwritten rows."""
    monkeypatch.setenv("SLAM2D_POISON", "1")
    return True


def dev(a):
    """The bytes of a host array on the device (one spare byte, so that an empty array still has an address)."""
    import torch

    b = np.ascontiguousarray(a).view(np.uint8).reshape(-1)
    return torch.from_numpy(np.concatenate([b, np.zeros(8, np.uint8)])).cuda()


def dpoison(shape, dtype):
    return dev(R.poisoned(shape, dtype))


def host(t, dtype, shape):
    n = int(np.prod(shape)) * np.dtype(dtype).itemsize
    return t.cpu().numpy()[:n].copy().view(dtype).reshape(shape)


def sync():
    import torch

    torch.cuda.synchronize()


def stage_of(params, max_jobs, max_links=64, max_matches=1, n_readings=12):
    return ke.LinkStage(ke.default_params(**params), n_readings, max_jobs, max_links, max_matches)


def gpu_add_edges(w, st=None, stream=0):
    """Stage 1 of a world: (links [J + 1, K], out [J], pool after); the context has one spare row."""
    J, K_ = len(w["jobs"]), int(w["max_links"])
    own = st is None
    st = stage_of(w["params"], J + 1, K_) if own else st
    chains = np.ascontiguousarray(w["near_chains"])
    d = {k: dev(w[k]) for k in ("jobs", "pool_poses", "seq", "running", "near", "near_source")}
    d_ch = dev(chains)
    sync()
    st.add_edges_device(J, d["jobs"].data_ptr(), d["pool_poses"].data_ptr(), len(w["pool_poses"]), d["seq"].data_ptr(),
                        len(w["seq"]), d["running"].data_ptr() if len(w["running"]) else 0, len(w["running"]),
                        d["near"].data_ptr() if len(w["near"]) else 0, d["near_source"].data_ptr() if len(w["near"]) else 0,
                        len(w["near"]), d_ch.data_ptr() if len(w["near"]) else 0, chains.shape[1], chains.shape[0],
                        int(w.get("flags", 0)), stream)
    links, out = st.get_links(0, J + 1)
    pool = host(d["pool_poses"], np.float64, w["pool_poses"].shape)
    if own:
        st.close()
    return links, out[:J], pool


def assert_stage1(w, want, what):
    links, out, pool = gpu_add_edges(w)
    J = len(w["jobs"])
    R.assert_same_records(links[:J], want[0], f"{what} links")
    R.assert_same_records(out, want[1], f"{what} out")
    R.assert_same_records(pool, want[2], f"{what} pool")
    assert links[J].tobytes() == R.poisoned(int(w["max_links"]), R.LINK).tobytes(), f"{what}: the row after the last job"


def gpu_loop_coarse(st, lw, stream=0):
    """ke_loop_coarse_device on a loop world: the dict R.loop_coarse gives, from poisoned device buffers."""
    M, cap, bcap, nr = len(lw["coarse"]), int(lw["capacity"]), int(lw["base_capacity"]), int(lw["n_readings"])
    d_in = {k: dev(lw[k]) for k in ("coarse", "query", "base_begin", "base_index", "pool_ranges")}
    d_n = dev(np.array([M], np.int32))
    o = dict(fq=dpoison(max(cap, 1), np.int32), fbb=dpoison(cap + 1, np.int32), fbi=dpoison(max(bcap, 1), np.int32),
             fof=dpoison(max(cap, 1), np.int32), nf=dpoison(1, np.int32), tr=dpoison((max(cap, 1), nr), np.float64),
             tp=dpoison((max(cap, 1), 3), np.float64))
    sync()
    st.loop_coarse_device(M, d_n.data_ptr(), d_in["coarse"].data_ptr(), d_in["query"].data_ptr(), d_in["base_begin"].data_ptr(),
                          d_in["base_index"].data_ptr(), d_in["pool_ranges"].data_ptr(), int(lw["pool_scans"]),
                          int(lw["tmp_first"]), cap, bcap, o["fq"].data_ptr(), o["fbb"].data_ptr(), o["fbi"].data_ptr(),
                          o["fof"].data_ptr(), o["nf"].data_ptr(), o["tr"].data_ptr(), o["tp"].data_ptr(), stream)
    info = st.loop_info()
    return dict(fine_query=host(o["fq"], np.int32, cap), fine_base_begin=host(o["fbb"], np.int32, cap + 1),
                fine_base_index=host(o["fbi"], np.int32, bcap), fine_of=host(o["fof"], np.int32, cap),
                n_fine=int(host(o["nf"], np.int32, 1)[0]), tmp_ranges=host(o["tr"], np.float64, (cap, nr)),
                tmp_poses=host(o["tp"], np.float64, (cap, 3)), info=info), (o, d_in)


def assert_coarse(got, want, what):
    assert got["n_fine"] == want["n_fine"] and tuple(got["info"]) == tuple(want["info"]), (what, got["n_fine"], got["info"], want["info"])
    for k in ("fine_query", "fine_base_begin", "fine_base_index", "fine_of"):
        np.testing.assert_array_equal(got[k], want[k], err_msg=f"{what} {k}")  # the poison beyond the count included
    for k in ("tmp_ranges", "tmp_poses"):
        R.assert_same_records(got[k], want[k], f"{what} {k}")


def gpu_loop_fine(st, lw, dbuf, fine, pool_poses=None, flags=0, stream=0):
    o, d_in = dbuf
    count = int(lw["count"])
    d_fine, d_src, d_ch = dev(fine), dev(lw["source"]), dev(np.ascontiguousarray(lw["loop_chains"]))
    d_cl = dpoison(count + 1, R.CLOSURE)
    d_pool = dev(pool_poses) if pool_poses is not None else None
    sync()
    st.loop_fine_device(count, int(lw["capacity"]), o["nf"].data_ptr(), d_fine.data_ptr(), o["fof"].data_ptr(),
                        len(lw["source"]), d_src.data_ptr(), d_in["query"].data_ptr(), d_ch.data_ptr(),
                        lw["loop_chains"].shape[1], d_cl.data_ptr(), d_pool.data_ptr() if d_pool is not None else 0,
                        len(pool_poses) if pool_poses is not None else 0, flags, stream)
    sync()
    cl = host(d_cl, R.CLOSURE, count + 1)
    assert cl[count].tobytes() == R.poisoned(1, R.CLOSURE).tobytes()
    return cl[:count], (host(d_pool, np.float64, pool_poses.shape) if d_pool is not None else None)


def loop_jobs(lw):
    """Stage 3's jobs, closest entries and pool poses for a loop world: slot s is scan 39 of graph s at pool offset
    40 s; every third slot's chain is too far to link."""
    rng = np.random.default_rng(77)
    count = int(lw["count"])
    jobs = ke.jobs([(s, 39, 40 * s, 38, 0, -1, 0, 0) for s in range(count)])
    closest = np.zeros(count, R.CLOSEST)
    closest["closest"] = rng.integers(0, 38, count)
    closest["linked"] = [0 if s % 3 == 2 else 1 for s in range(count)]
    pool = rng.uniform(-6, 6, (int(lw["pool_scans"]), 3))
    pool[0] = 0.0  # a from-scan at the origin
    return jobs, closest, pool


def assert_loop_world(lw, what, flags=ke.KE_WRITE_POSE):
    st = stage_of(lw["params"], int(lw["count"]) + 1, 2, len(lw["coarse"]), int(lw["n_readings"]))
    want_co = R.loop_coarse(lw)
    got_co, dbuf = gpu_loop_coarse(st, lw)
    assert_coarse(got_co, want_co, what)
    fine = K.fine_results(np.random.default_rng(5), lw, want_co["fine_of"], want_co["n_fine"])
    jobs, closest, pool = loop_jobs(lw)
    want_cl, want_pool = R.loop_fine(lw, want_co["fine_of"], want_co["n_fine"], fine, pool, flags)
    got_cl, got_pool = gpu_loop_fine(st, lw, dbuf, fine, pool, flags)
    R.assert_same_records(got_cl, want_cl, f"{what} closures")
    R.assert_same_records(got_pool, want_pool, f"{what} pool after the fine call")
    # stage 3 on those closures
    want_links, want_out = R.close(jobs, want_cl, closest, want_pool, 2)
    count = len(jobs)
    d_jobs, d_cl, d_cs, d_pool = dev(jobs), dev(want_cl), dev(closest), dev(want_pool)
    sync()
    st.close_device(count, d_jobs.data_ptr(), d_cl.data_ptr(), d_cs.data_ptr(), d_pool.data_ptr(), len(want_pool))
    links, out = st.get_links(0, count + 1)
    R.assert_same_records(links[:count], want_links, f"{what} KE_LOOP records")
    R.assert_same_records(out[:count], want_out, f"{what} close out")
    assert links[count].tobytes() == R.poisoned(2, R.LINK).tobytes()
    st.close()
    return want_cl, want_out


# ------------------------------------------------------------------------------------ 1. directed cases and the golden
@pytest.mark.parametrize("name", list(K.stage1_cases()) + ["bad_indices"])
def test_stage1_directed_case(poison, name):
    w = K.case_bad_indices() if name == "bad_indices" else K.stage1_cases()[name]
    assert_stage1(w, R.add_edges(w), name)


@pytest.mark.parametrize("name", list(K.loop_cases()))
def test_loop_directed_case(poison, name):
    cl, out = assert_loop_world(K.loop_cases()[name], name)
    if name == "fine_edges":
        assert cl["chain"].tolist() == [0, 1, -1, 2] and out["n_links"].tolist() == [1, 1, 0, 1]
    assert_loop_world(K.loop_cases()[name], name + " without KE_WRITE_POSE", flags=0)


def test_golden_fixture(poison):
    """The fixture's expected records come from the plain transcription: the GPU equals them directly."""
    stage1, loops = G.load()
    for name, (w, want_links, want_out, want_pool) in stage1.items():
        assert_stage1(w, (want_links, want_out, want_pool), f"golden {name}")
    for name, (lw, want_of, want_closing) in loops.items():
        st = stage_of(lw["params"], lw["count"] + 1, 2, len(lw["coarse"]), lw["n_readings"])
        co, dbuf = gpu_loop_coarse(st, lw)
        assert co["info"][0] == len(want_of)
        np.testing.assert_array_equal(co["fine_of"][:co["n_fine"]], want_of[:co["n_fine"]], err_msg=name)
        fine = K.fine_results(np.random.default_rng(1), lw, co["fine_of"], co["n_fine"])
        cl, _ = gpu_loop_fine(st, lw, dbuf, fine)
        if co["n_fine"] == len(want_of):
            np.testing.assert_array_equal(cl["chain"], want_closing, err_msg=name)
        st.close()


# ------------------------------------------------------------------------------------ 2. launch shapes
def shape_world(n_jobs: int) -> dict:
    """Mixed link counts 0 .. 64 over the jobs, one KE_ERANGE job among the good ones from 3 jobs on."""
    rng = np.random.default_rng(200 + n_jobs)
    counts = [0, 1, 2, 5, 17, 64, 3, 33, 63, 9]
    specs = [K.links_spec(rng, counts[j % len(counts)] if j % 50 < 10 else int(rng.integers(0, 7)), S=12) for j in range(n_jobs)]
    if n_jobs >= 3:
        specs[n_jobs // 2] = K.links_spec(rng, 65, S=12)
    return K.build_world(specs, flags=R.KE_WRITE_POSE)


@pytest.mark.parametrize("n_jobs", [1, 3, 4, 5, 257, 1000])
def test_launch_shapes(poison, n_jobs):
    """A partial last workgroup (four jobs per workgroup) and many workgroups."""
    w = shape_world(n_jobs)
    want = R.add_edges(w)
    assert (want[1]["status"] == R.KE_ERANGE).sum() == (1 if n_jobs >= 3 else 0)
    assert n_jobs < 257 or {0, 1, 64} <= set(want[1]["n_links"].tolist())
    assert_stage1(w, want, f"{n_jobs} jobs")


# ------------------------------------------------------------------------------------ 3. coarse compaction
def compaction_world(n_matches: int, capacity: int, accept=0.6) -> dict:
    rng = np.random.default_rng(300 + n_matches)
    slots, left = [], n_matches
    while left > 0:
        n = min(left, int(rng.integers(1, 6)))
        slots.append([dict(coarse=K.OK_C if rng.random() < accept else (0.3, 0.01, 0.01), fine=0.9,
                           length=int(rng.integers(1, 5))) for _ in range(n)])
        left -= n
    return K.build_loop_world(rng, slots, capacity=capacity, n_readings=5)


@pytest.mark.parametrize("n_matches", [1, 63, 64, 65, 1025])
def test_coarse_compaction(poison, n_matches):
    """Order, base lists and d_fine_of over one and several 256-match rounds of the prefix sum, with the capacity
    above, at and below the accepted count."""
    accepted = R.loop_coarse(compaction_world(n_matches, n_matches))["n_fine"]
    for cap in sorted({n_matches, accepted, max(accepted - 1, 0), accepted // 2}):
        lw = compaction_world(n_matches, cap)
        want = R.loop_coarse(lw)
        assert want["info"][0] == accepted and want["n_fine"] == min(cap, accepted)
        st = stage_of(lw["params"], 1, 1, n_matches, 5)
        got, _ = gpu_loop_coarse(st, lw)
        assert_coarse(got, want, f"{n_matches} matches, capacity {cap}")
        st.close()
    lw = compaction_world(n_matches, n_matches, accept=1.0)  # every match accepted
    st = stage_of(lw["params"], 1, 1, n_matches, 5)
    got, _ = gpu_loop_coarse(st, lw)
    assert_coarse(got, R.loop_coarse(lw), f"{n_matches} matches, all accepted")
    assert got["fine_of"].tolist() == list(range(n_matches))
    st.close()


# ------------------------------------------------------------------------------------ 4. one step on two ring graphs
N_RING, RADIUS = 40, 3.0
KL_PRM = dict(link_scan_maximum_distance=1.5, loop_search_maximum_distance=4.0, loop_match_minimum_chain_size=3,
              use_scan_barycenter=0)
LASER = dict(minimum_angle=-1.0, angular_resolution=0.25, minimum_range=0.1, range_threshold=12.0, n_readings=8)
OFFSETS = (4, 4 + N_RING)
TMP_FIRST, CAPACITY = 4 + 2 * N_RING, 4
RUNNING = (29, 10)  # the running scans: [29, 39)


class PlainSide:
    """The same step by the transcriptions: karto_loop_plain's graph and search, karto_link_plain's records, the SPA
    restatement.  One instance per graph."""

    def __init__(self, poses, early_edges):
        self.poses = np.array(poses, np.float64)
        self.g, self.spa = LP.Graph(), SR.RefGraph()
        self.n_cons = 0
        for i in range(N_RING - 1):
            self.add_scan(i)
            if i:
                self.link(i - 1, i, self.poses[i], setup_cov(i))
        for a, b in early_edges:
            self.link(a, b, self.poses[b], setup_cov(a + b))

    def add_scan(self, i):
        assert self.g.add_vertex() == i
        self.spa.add_node(i, self.poses[i])

    def link(self, a, b, mean, cov):
        """LinkScans."""
        _, new = self.g.add_edge(a, b)
        if new:
            li = P.LinkInfo(P.Pose2(*self.poses[a]), P.Pose2(*mean), P.Matrix3(cov))
            assert self.spa.add_constraint(a, b, li.pose_difference.tolist(), P.precision_matrix(li).tolist())
            self.n_cons += 1
        return new

    def ref(self):
        return [(float(x), float(y)) for x, y in self.poses[:len(self.g.vertices), :2]]

    def ends(self):
        return [(e.source.obj, e.target.obj) for e in self.g.edges]

    def optimise(self):
        self.spa.compute()
        self.poses[:len(self.spa.poses)] = np.asarray(self.spa.poses)


def setup_cov(k):
    return K.spd(np.random.default_rng(900 + k), 0.002)


def ring_poses(seed):
    rng = np.random.default_rng(seed)
    return SR.ring_truth(N_RING, RADIUS) + rng.normal(0.0, [0.01, 0.01, 0.005], (N_RING, 3))


def test_one_process_step_on_two_ring_graphs(gpu):
    """kl_search -> kl_emit -> synthetic results -> ke_add_edges -> ke_commit -> spa_compute, then the loop stages ->
    ke_close -> ke_commit -> spa_compute, for a fleet of two 40-scan rings: graph 0 has an earlier closure edge (near
    chains, no loop candidate), graph 1 none (a loop candidate, no near chain).  Edge lists, constraint counts and
    final poses equal the transcriptions'."""
    import torch

    S = N_RING - 1  # the new scan
    early = [[(1, S - 1)], []]
    plain = [PlainSide(ring_poses(41 + g), early[g]) for g in range(2)]
    laser = KtLaser(*[LASER[k] for k in ("minimum_angle", "angular_resolution", "minimum_range", "range_threshold", "n_readings")], 0)
    f = kl.LoopSearchFleet(laser, kl.default_params(**KL_PRM), 2, N_RING + 5, 200, 4)
    spa = SpaFleet(2, N_RING + 5, 200)
    st = ke.LinkStage(ke.default_params(), LASER["n_readings"], 4, 8, 16)
    P_ = TMP_FIRST + CAPACITY
    pool = np.zeros((P_, 3))
    ranges = np.full((P_, LASER["n_readings"]), 5.0)
    for g in range(2):
        f.set_pool_offset(g, OFFSETS[g])
        pl = plain[g]
        for i in range(S):
            assert f.add_vertex(g) == i
            spa.add_node(g, i, pl.poses[i])
        for a, b in pl.ends():
            assert f.add_edge(g, a, b)
        for (a, b), m, p in zip(pl.spa.ends, pl.spa.means, pl.spa.precs):
            assert spa.add_constraint(g, pl.spa.ids[a], pl.spa.ids[b], m, p)
        # Mapper::Process: AddVertex / AddNode for the new scan
        pl.add_scan(S)
        assert f.add_vertex(g) == S
        spa.add_node(g, S, pl.poses[S])
        pool[OFFSETS[g]:OFFSETS[g] + N_RING] = pl.poses
    d_pool, d_ranges = torch.from_numpy(pool).cuda(), torch.from_numpy(ranges).cuda()
    sync()

    def refresh(first, count):
        for g in range(2):
            o = OFFSETS[g] + first
            f.set_scans_device(g, first, count, d_ranges[o:].data_ptr(), d_pool[o:].data_ptr())

    refresh(0, N_RING)
    rng = np.random.default_rng(4)
    seq = R.results([plain[g].poses[S] for g in range(2)], [K.spd(rng, 0.003) for _ in range(2)], [0.9, 0.9])
    d_seq = dev(seq)
    # the running scans' closest scan
    items = np.array([(g, S, RUNNING[0], RUNNING[1]) for g in range(2)], np.int32)
    d_items, d_running = dev(items), dpoison(2, R.CLOSEST)
    sync()
    f.closest_device(2, d_items.data_ptr(), d_running.data_ptr())
    sync()
    running = host(d_running, R.CLOSEST, 2)
    rd = f.result_device()

    def add_edges(jobs, d_near, d_src, n_near, flags):
        d_jobs = dev(jobs)
        sync()
        st.add_edges_device(len(jobs), d_jobs.data_ptr(), d_pool.data_ptr(), P_, d_seq.data_ptr(), 2, d_running.data_ptr(), 2,
                            d_near, d_src, n_near, rd["near_chains"], rd["chain_stride"], 2, flags)

    # LinkScans(prev) and the running scans' link come first in AddEdges: FindNearChains' traversal starts at the new
    # vertex and runs over these edges.  The running chain's closest scan is the previous scan: one edge, one constraint
    # (without KE_WRITE_POSE: the pose is set by the full call below)
    add_edges(ke.jobs([(g, S, OFFSETS[g], S - 1, g, g, 0, 0) for g in range(2)]), 0, 0, 0, 0)
    assert st.commit(f, spa, 0, 2) == 2
    for g in range(2):
        pl = plain[g]
        rcov = seq[g]["covariance"]
        assert pl.link(S - 1, S, pl.poses[S], rcov)
        closest, linked = LP.link_test(pl.ref(), list(range(RUNNING[0], RUNNING[0] + RUNNING[1])), S, KL_PRM["link_scan_maximum_distance"])
        assert (closest, linked) == (S - 1, 1) == tuple(running[g])
        assert not pl.link(closest, S, pl.poses[S], rcov)
    np.testing.assert_array_equal(R.bits(d_pool.cpu().numpy()), R.bits(pool))  # nothing written without the flag

    def searched(which, capacity=8):
        f.search([(g, S, 0, -1, -1) for g in range(2)])
        o = dict(q=dpoison(capacity, np.int32), bb=dpoison(capacity + 1, np.int32), bi=dpoison(2 * (N_RING + 5), np.int32),
                 src=dpoison(capacity, R.SOURCE), n=dpoison(1, np.int32))
        sync()
        f.emit_batch_device(2, which, capacity, o["q"].data_ptr(), o["bb"].data_ptr(), o["bi"].data_ptr(), o["src"].data_ptr(),
                            o["n"].data_ptr())
        sync()
        n = int(host(o["n"], np.int32, 1)[0])
        return o, n, host(o["src"], R.SOURCE, capacity)[:n]

    # ---- LinkNearChains
    o, n_near, src = searched(kl.KL_NEAR_CHAINS)
    want_chains = []
    for g in range(2):
        pl = plain[g]
        chains = [c for c in LP.find_near_chains(pl.g, pl.ref(), S, KL_PRM["link_scan_maximum_distance"]) if len(c) >= 3]
        want_chains.append(chains)
    assert [len(c) for c in want_chains] == [1, 0] and n_near == 1 and src["slot"].tolist() == [0]
    near = R.results([plain[0].poses[S] + [0.02, -0.01, 0.004]], [K.spd(rng, 0.004)], [0.93])
    d_near = dev(near)
    jobs = ke.jobs([(0, S, OFFSETS[0], S - 1, 0, 0, 0, 1), (1, S, OFFSETS[1], S - 1, 1, 1, 1, 0)])
    add_edges(jobs, d_near.data_ptr(), o["src"].data_ptr(), n_near, ke.KE_WRITE_POSE)
    links, out = st.get_links(0, 2)
    assert out["n_links"].tolist() == [3, 2] and out["n_means"].tolist() == [2, 1] and not out["status"].any()
    assert st.commit(f, spa, 0, 2) == 1  # the KE_PREV and KE_RUNNING records are old edges now: only 0 -> 39 is new
    assert st.commit(f, spa, 0, 2) == 0  # and a second commit is a no-op
    for g in range(2):
        pl = plain[g]
        rcov = P.Matrix3(seq[g]["covariance"])
        means, covs = [P.Pose2(*pl.poses[S])], [rcov]
        for chain in want_chains[g]:
            means.append(P.Pose2(*near[0]["mean"]))
            covs.append(P.Matrix3(near[0]["covariance"]))
            closest, linked = LP.link_test(pl.ref(), chain, S, KL_PRM["link_scan_maximum_distance"])
            assert linked and pl.link(closest, S, near[0]["mean"], near[0]["covariance"])
        pl.poses[S] = P.compute_weighted_mean(means, covs).tolist()  # pScan->SetSensorPose
        np.testing.assert_array_equal(R.bits(out[g]["pose"]), R.bits(pl.poses[S]))
    got_pool = d_pool.cpu().numpy()
    for g in range(2):
        np.testing.assert_array_equal(R.bits(got_pool[OFFSETS[g] + S]), R.bits(plain[g].poses[S]))

    def compare_graphs(what):
        for g in range(2):
            pl = plain[g]
            assert f.counts(g) == (N_RING, len(pl.ends())), what
            assert spa.counts(g) == (N_RING, pl.n_cons), what
        spa.compute(0, 2)
        for g in range(2):
            plain[g].optimise()
            ids, poses = spa.get_nodes(g)
            np.testing.assert_array_equal(R.bits(poses), R.bits(plain[g].poses), err_msg=f"{what} graph {g}")
            d_pool[OFFSETS[g]:OFFSETS[g] + N_RING] = torch.from_numpy(poses).cuda()  # CorrectPoses
        sync()
        refresh(0, N_RING)

    compare_graphs("after AddEdges")

    # ---- TryCloseLoop
    o, n_coarse, src = searched(kl.KL_LOOP_CHAINS)
    want_loop = [LP.loop_chains(plain[g].g, plain[g].ref(), S, 0, KL_PRM["loop_search_maximum_distance"], 3) for g in range(2)]
    assert [len(c) for c in want_loop] == [0, 1] and n_coarse == 1 and src["slot"].tolist() == [1]
    coarse = R.results([plain[1].poses[S] + [0.05, 0.03, -0.01]], [K.spd(rng, 0.004)], [0.9])
    d_coarse = dev(coarse)
    fo = dict(fq=dpoison(CAPACITY, np.int32), fbb=dpoison(CAPACITY + 1, np.int32), fbi=dpoison(2 * (N_RING + 5), np.int32),
              fof=dpoison(CAPACITY, np.int32), nf=dpoison(1, np.int32))
    d_tmp_ranges, d_tmp_poses = d_ranges[TMP_FIRST:], d_pool[TMP_FIRST:]
    sync()
    st.loop_coarse_device(8, o["n"].data_ptr(), d_coarse.data_ptr(), o["q"].data_ptr(), o["bb"].data_ptr(), o["bi"].data_ptr(),
                          d_ranges.data_ptr(), P_, TMP_FIRST, CAPACITY, 2 * (N_RING + 5), fo["fq"].data_ptr(),
                          fo["fbb"].data_ptr(), fo["fbi"].data_ptr(), fo["fof"].data_ptr(), fo["nf"].data_ptr(),
                          d_tmp_ranges.data_ptr(), d_tmp_poses.data_ptr())
    assert st.loop_info() == (1, 0) and int(host(fo["nf"], np.int32, 1)[0]) == 1
    begin, length, resume = want_loop[1][0]
    fbb = host(fo["fbb"], np.int32, CAPACITY + 1)
    assert host(fo["fbi"], np.int32, 2 * (N_RING + 5))[fbb[0]:fbb[1]].tolist() == [OFFSETS[1] + begin + i for i in range(length)]
    assert host(fo["fq"], np.int32, CAPACITY)[0] == TMP_FIRST
    tmp = d_pool.cpu().numpy()[TMP_FIRST:]
    np.testing.assert_array_equal(R.bits(tmp[0]), R.bits(coarse[0]["mean"]))
    assert not tmp[1:].any() and np.isinf(d_ranges.cpu().numpy()[TMP_FIRST + 1:]).all()
    fine = R.results([plain[1].poses[S] + [0.04, 0.02, -0.008]], [K.spd(rng, 0.002)], [0.88])
    d_fine, d_cl = dev(fine), dpoison(2, R.CLOSURE)
    sync()
    st.loop_fine_device(2, CAPACITY, fo["nf"].data_ptr(), d_fine.data_ptr(), fo["fof"].data_ptr(), 8, o["src"].data_ptr(),
                        o["q"].data_ptr(), rd["loop_chains"], rd["chain_stride"], d_cl.data_ptr(), d_pool.data_ptr(), P_,
                        ke.KE_WRITE_POSE)
    sync()
    cl = host(d_cl, R.CLOSURE, 2)
    assert cl["chain"].tolist() == [-1, 0] and cl["resume"].tolist() == [-1, resume]
    matched, closed = P.try_close_loop(K.DEFAULT_PARAMS, [(coarse[0], fine[0])])
    assert (matched, closed) == ([0], 0)
    plain[1].poses[S] = fine[0]["mean"]  # pScan->SetSensorPose(bestPose)
    np.testing.assert_array_equal(R.bits(d_pool.cpu().numpy()[OFFSETS[1] + S]), R.bits(fine[0]["mean"]))
    refresh(S, 1)
    items = np.array([(0, S, 0, 0), (1, S, begin, length)], np.int32)  # slot 0 has no closure: an empty chain
    d_items, d_closest = dev(items), dpoison(2, R.CLOSEST)
    sync()
    f.closest_device(2, d_items.data_ptr(), d_closest.data_ptr())
    d_jobs = dev(ke.jobs([(g, S, OFFSETS[g], S - 1, g, -1, 0, 0) for g in range(2)]))
    sync()
    st.close_device(2, d_jobs.data_ptr(), d_cl.data_ptr(), d_closest.data_ptr(), d_pool.data_ptr(), P_)
    links, out = st.get_links(0, 2)
    closest, linked = LP.link_test(plain[1].ref(), list(range(begin, begin + length)), S, KL_PRM["link_scan_maximum_distance"])
    assert linked and out["n_links"].tolist() == [0, 1] and (links[1, 0]["from"], links[1, 0]["to"], links[1, 0]["kind"]) == (closest, S, ke.KE_LOOP)
    assert st.commit(f, spa, 0, 2) == 1
    assert st.commit(f, spa, 0, 2) == 0
    assert plain[1].link(closest, S, fine[0]["mean"], fine[0]["covariance"])
    compare_graphs("after the closure")
    assert [f.counts(g)[1] for g in range(2)] == [N_RING - 2 + 1 + 2, N_RING - 2 + 2]
    st.close()
    spa.close()
    f.close()


# ------------------------------------------------------------------------------------ 5. streams and timing
def test_caller_stream_and_timing(poison):
    import torch

    w = K.case_link_counts()
    lw = K.loop_cases()["fine_edges"]
    want = R.add_edges(w)
    s = torch.cuda.Stream()
    J = len(w["jobs"])
    st = stage_of(w["params"], J + 1, 64, len(lw["coarse"]))
    st.set_timing(True)
    with torch.cuda.stream(s):
        links, out, pool = gpu_add_edges(w, st, s.cuda_stream)
        got_co, dbuf = gpu_loop_coarse(st, lw, s.cuda_stream)
        fine = K.fine_results(np.random.default_rng(5), lw, got_co["fine_of"], got_co["n_fine"])
        cl, _ = gpu_loop_fine(st, lw, dbuf, fine, stream=s.cuda_stream)
        jobs, closest, pl = loop_jobs(lw)
        d = [dev(v) for v in (jobs, cl, closest, pl)]
        s.synchronize()
        st.close_device(len(jobs), d[0].data_ptr(), d[1].data_ptr(), d[2].data_ptr(), d[3].data_ptr(), len(pl), s.cuda_stream)
        s.synchronize()  # the calls completed on the caller's stream: nothing else is waited for
    R.assert_same_records(links[:J], want[0], "links on a caller's stream")
    R.assert_same_records(out, want[1], "out on a caller's stream")
    assert_coarse(got_co, R.loop_coarse(lw), "coarse on a caller's stream")
    assert cl["chain"].tolist() == [0, 1, -1, 2]
    times = st.kernel_times(reset=True)
    assert {k: v[1] for k, v in times.items()} == {"ke_add_edges_kernel": 1, "ke_coarse_scan_kernel": 1,
                                                   "ke_coarse_write_kernel": 1, "ke_fine_kernel": 1, "ke_close_kernel": 1}
    assert all(v[0] > 0.0 for v in times.values())
    assert all(v == (0.0, 0) for v in st.kernel_times().values())
    st.set_timing(False)
    gpu_add_edges(w, st)
    assert all(v == (0.0, 0) for v in st.kernel_times().values())
    st.close()
