"""Directed and random cases of the Karto graph-linking stage (include/slam2d/karto_link.h) for the tests.

A stage-1 WORLD is the set of device inputs of one ke_add_edges_device call, built from one spec per job:
  dict(poses [S, 3]           the graph's sensor poses; the job's scan is the last one, S - 1
       prev bool              a previous scan S - 2 exists (False: a graph's first scan, prev = -1)
       rcov [9]               the sequential match's covariance
       running None | (closest, linked)
       near  list of dict(response, mean [3], cov [9], closest, linked))
Graph g's scans are pool slots [g * S_max, ...); job j searches in slot j and its near matches are consecutive in the
near batch, as kl_emit_batch_device orders them.  A LOOP WORLD is the input of the stage-2 calls.
Test infrastructure: nothing here is imported by the package.
"""
from __future__ import annotations

import math

import numpy as np

import karto_link_ref as R

DEFAULT_PARAMS = dict(link_match_minimum_response_fine=0.8, loop_match_minimum_response_coarse=0.8,
                      loop_match_maximum_variance_coarse=0.4 * 0.4, loop_match_minimum_response_fine=0.8)
NODE_PARAMS = dict(link_match_minimum_response_fine=0.1, loop_match_minimum_response_coarse=0.35,
                   loop_match_maximum_variance_coarse=3.0 * 3.0, loop_match_minimum_response_fine=0.45)

SINGULAR_COV = [1.0, 2.0, 0.0, 2.0, 4.0, 0.0, 0.0, 0.0, 1.0]  # rows 0 and 1 dependent: fDet = 0
NAN_COV = [math.nan, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 1.0]


def spd(rng, scale=None):
    """A random symmetric positive-definite covariance, row-major [9]."""
    a = rng.normal(size=(3, 3))
    s = 10.0 ** rng.uniform(-3, -1) if scale is None else scale
    return ((a @ a.T + 0.3 * np.eye(3)) * s).reshape(9)


def threshold(params) -> float:
    return params["link_match_minimum_response_fine"] - R.KL_TOLERANCE


def build_world(specs, params=None, max_links=64, flags=0, chain_stride=None) -> dict:
    params = dict(DEFAULT_PARAMS if params is None else params)
    J = len(specs)
    S = max(len(np.reshape(s["poses"], (-1, 3))) for s in specs)
    n_near = sum(len(s["near"]) for s in specs)
    stride = max([2 * len(s["near"]) + 1 for s in specs] + [2]) if chain_stride is None else chain_stride
    pool = np.zeros((J * S, 3))
    jobs = np.zeros(J, R.JOB)
    seq = np.zeros(J, R.KT_RESULT)
    running = []
    near = np.zeros(n_near, R.KT_RESULT)
    src = np.zeros(n_near, R.SOURCE)
    chains = np.zeros((J, stride), R.NEAR_CHAIN)
    chains["closest"] = -7  # an entry no accepted match names is never followed
    m = 0
    for j, s in enumerate(specs):
        po = np.reshape(np.asarray(s["poses"], np.float64), (-1, 3))
        n = len(po)
        pool[j * S:j * S + n] = po
        # the sequential result sits at a permuted index, so that seq_result is really followed
        q = (j * 7 + 3) % J if math.gcd(7, J) == 1 else j
        seq[q]["covariance"] = s.get("rcov", np.eye(3).reshape(9) * 0.01)
        seq[q]["mean"] = po[n - 1]
        seq[q]["response"] = 0.9
        run = -1
        if s.get("running") is not None:
            run = len(running)
            running.append(tuple(int(v) for v in s["running"]))
        jobs[j] = (j, n - 1, j * S, n - 2 if s["prev"] else -1, q, run, m, len(s["near"]))
        for k, e in enumerate(s["near"]):
            near[m]["response"] = e["response"]
            near[m]["mean"] = e["mean"]
            near[m]["covariance"] = e["cov"]
            src[m] = (j, 2 * k + 1)  # the long chains among all near chains: every other one
            chains[j, 2 * k + 1] = (0, 5, e["closest"], R.KL_CHAIN_LONG | (R.KL_CHAIN_LINKED if e["linked"] else 0))
            m += 1
    return dict(jobs=jobs, pool_poses=pool, seq=seq, running=np.array(running, R.CLOSEST).reshape(-1), near=near,
                near_source=src, near_chains=chains, params=params, max_links=max_links, flags=flags)


def near_entry(rng, S, response=0.95, linked=True, cov=None, around=None):
    centre = np.zeros(3) if around is None else np.asarray(around)
    mean = centre + rng.normal(size=3) * [0.05, 0.05, 0.02]
    return dict(response=response, mean=mean, cov=spd(rng) if cov is None else cov, closest=int(rng.integers(0, S - 2)),
                linked=linked)


def walk(rng, S, start=None, heading_scale=1.0):
    """S sensor poses along a random walk."""
    po = np.zeros((S, 3))
    po[0] = rng.uniform(-5, 5, 3) if start is None else start
    for k in range(1, S):
        h = po[k - 1, 2]
        step = rng.uniform(0.2, 0.6)
        po[k] = [po[k - 1, 0] + step * math.cos(h), po[k - 1, 1] + step * math.sin(h),
                 po[k - 1, 2] + rng.normal() * 0.3 * heading_scale]
    return po


def spec(rng, S=8, prev=True, running=(0, 1), n_near=2, **kw):
    po = walk(rng, S, kw.get("start"))
    return dict(poses=po, prev=prev, rcov=spd(rng), running=running,
                near=[near_entry(rng, S, around=po[-1]) for _ in range(n_near)])


def find_one_minus_c_heading():
    """A heading h whose rotation by -h has (1 - c) + c != 1.0: FromAxisAngle's [2][2] taken literally is not 1."""
    for k in range(1, 4000):
        h = k * 0.001
        c = R.cos(-h)
        if (1.0 - c) + c != 1.0:
            return h
    raise AssertionError("no heading with (1 - c) + c != 1.0 found")


# ------------------------------------------------------------------------------------------------ stage 1, directed
def case_set_transform():
    """pose1 == Pose2() exactly; pose1 at the origin position with a heading; -0.0 components; the general case."""
    rng = np.random.default_rng(11)
    specs = []
    for p1 in ([0.0, 0.0, 0.0], [0.0, 0.0, 0.7], [-0.0, 0.0, -0.0], [0.0, -0.0, -2.5], [1.5, -0.25, 0.4], [0.0, 2.0, 0.0]):
        s = spec(rng, S=4, running=(2, 1), n_near=1)
        s["poses"][2] = p1          # the previous scan and the running chain's closest scan
        s["near"][0]["closest"] = 2
        specs.append(s)
    return build_world(specs)


def case_big_headings():
    """Headings beyond +-2 pi in the from-scan, the scan and the means: NormalizeAngle's cast branches, both signs,
    in the pose difference and in the weighted mean's accumulation."""
    rng = np.random.default_rng(12)
    specs = []
    for h1, h2 in ((7.5, -7.0), (-13.2, 14.0), (20.0, 0.1), (-0.1, -20.0), (3.2, -3.2), (40.0, -45.0)):
        s = spec(rng, S=4, running=(1, 1), n_near=2)
        s["poses"][2, 2] = h1
        s["poses"][3, 2] = h2
        s["near"][0]["mean"][2] = h2 + 6.5
        s["near"][1]["mean"][2] = -h2 * 3.0 - 9.0
        s["near"][0]["mean"][0] += 300.0  # a weight times a large pose: a large heading term in the accumulation
        specs.append(s)
    return build_world(specs)


def case_one_minus_c():
    rng = np.random.default_rng(13)
    h = find_one_minus_c_heading()
    s = spec(rng, S=4, running=None, n_near=1)
    s["poses"][2] = [0.4, -0.3, h]
    s["near"][0]["closest"] = 2
    return build_world([s])


def case_threshold(params=None):
    """Near responses exactly at link_min - KL_TOLERANCE (not accepted: the test is >) and one ulp above (accepted),
    one ulp below, and at link_min itself."""
    params = dict(DEFAULT_PARAMS if params is None else params)
    rng = np.random.default_rng(14)
    thr = threshold(params)
    s = spec(rng, S=6, n_near=5)
    for e, r in zip(s["near"], (thr, np.nextafter(thr, math.inf), np.nextafter(thr, -math.inf),
                                params["link_match_minimum_response_fine"], math.nan)):
        e["response"] = r
    return build_world([s, spec(rng, S=6, n_near=1)], params)


def case_singular():
    """A singular and a NaN covariance: as a near match's (its record is KE_SINGULAR and so is the mean), as the
    sequential match's, and a sum of inverses that is singular although every item inverts."""
    rng = np.random.default_rng(15)
    a = spec(rng, S=5, n_near=3)
    a["near"][1]["cov"] = SINGULAR_COV
    b = spec(rng, S=5, n_near=2)
    b["near"][0]["cov"] = NAN_COV
    c = spec(rng, S=5, n_near=1)
    c["rcov"] = SINGULAR_COV
    d = spec(rng, S=5, n_near=1)
    d["rcov"] = [1e-3, 0, 0, 0, 1e-3, 0, 0, 0, 1e-3]
    d["near"][0]["cov"] = [-1e-3, 0, 0, 0, 1e-3, 0, 0, 0, 1e-3]  # inverts; the sum's [0][0] is 1000 - 1000
    e = spec(rng, S=5, n_near=2)                                     # a not-accepted singular match is never inverted
    e["near"][0]["cov"] = SINGULAR_COV
    e["near"][0]["response"] = 0.2
    return build_world([a, b, c, d, e, spec(rng, S=5, n_near=1)])


def case_first_scan():
    """prev = -1: no KE_PREV, no KE_RUNNING (the running entry is not read), the mean list is the near matches only;
    and with no accepted match the pose stays."""
    rng = np.random.default_rng(16)
    a = spec(rng, S=3, prev=False, running=(0, 1), n_near=2)
    b = spec(rng, S=3, prev=False, running=None, n_near=1)
    b["near"][0]["response"] = 0.1
    c = spec(rng, S=1, prev=False, running=None, n_near=0)
    return build_world([a, b, c])


def links_spec(rng, n_links, S=70):
    """A job with exactly n_links records: KE_PREV, KE_RUNNING, then linked near matches, unlinked and rejected ones
    between them."""
    n_near = max(n_links - 2, 0)
    s = spec(rng, S=S, prev=n_links >= 1, running=(int(rng.integers(0, S - 2)), 1 if n_links >= 2 else 0), n_near=0)
    for k in range(n_near):
        s["near"].append(near_entry(rng, S, around=s["poses"][-1]))
        if k % 5 == 2:
            s["near"].append(near_entry(rng, S, linked=False, around=s["poses"][-1]))
        if k % 7 == 3:
            s["near"].append(near_entry(rng, S, response=0.3, around=s["poses"][-1]))
    return s


def case_link_counts():
    """0, 1, 2, 63, 64 and 65 links in one launch (65: KE_ERANGE, its row untouched), then a good job again; a first
    scan with 64 near links; and more than 64 near matches of which few are linked."""
    rng = np.random.default_rng(17)
    specs = [links_spec(rng, n) for n in (0, 1, 2, 63, 64, 65, 3)]
    first = spec(rng, S=70, prev=False, running=None, n_near=64)
    many = spec(rng, S=70, n_near=0)
    many["near"] = [near_entry(rng, 70, linked=k % 30 == 0, response=0.95 if k % 3 else 0.5, around=many["poses"][-1])
                    for k in range(150)]
    return build_world(specs + [first, many])


def case_small_rows():
    """max_links = 3: a job needing 4 is refused, one needing 3 is not."""
    rng = np.random.default_rng(18)
    return build_world([links_spec(rng, n, S=10) for n in (3, 4, 2, 0)], max_links=3)


def case_write_pose():
    """KE_WRITE_POSE: the weighted mean lands in the pool at the scan's slot; a refused, a singular and an
    empty-list job leave it alone."""
    rng = np.random.default_rng(19)
    sing = spec(rng, S=5, n_near=1)
    sing["near"][0]["cov"] = SINGULAR_COV
    empty = spec(rng, S=5, prev=False, running=None, n_near=0)
    return build_world([spec(rng, S=5), sing, empty, links_spec(rng, 5, S=9)], flags=R.KE_WRITE_POSE, max_links=4)


def case_node_params():
    rng = np.random.default_rng(20)
    s = spec(rng, S=6, n_near=4)
    for e, r in zip(s["near"], (0.05, 0.0999989, 0.0999991, 0.5)):
        e["response"] = r
    return build_world([s], NODE_PARAMS)


def case_bad_indices():
    """Every index a job names, out of range one job at a time: KE_EINVAL for that job, nothing of it written, the
    good jobs around it untouched.  (Not in the plain transcription: the reference has pointers, not indices.)"""
    rng = np.random.default_rng(21)
    w = build_world([spec(rng, S=5, n_near=2) for _ in range(12)])
    j, P = w["jobs"], len(w["pool_poses"])
    j[1]["scan"] = -1
    j[2]["pool_offset"] = P  # the scan's slot beyond the pool
    j[3]["prev"] = P         # the previous scan's slot beyond the pool
    j[4]["seq_result"] = len(w["seq"])
    j[5]["running"] = len(w["running"])
    j[6]["near_count"] = len(w["near"])  # runs past the batch's end
    j[7]["near_first"] = -1
    w["near_source"][j[8]["near_first"]]["slot"] = len(w["jobs"])
    w["near_source"][j[9]["near_first"] + 1]["chain"] = w["near_chains"].shape[1]
    w["near_chains"][10, 1]["closest"] = -1
    w["running"][j[11]["running"]]["closest"] = P
    return w


def stage1_cases() -> dict:
    return {"set_transform": case_set_transform(), "big_headings": case_big_headings(), "one_minus_c": case_one_minus_c(),
            "threshold": case_threshold(), "singular": case_singular(), "first_scan": case_first_scan(),
            "link_counts": case_link_counts(), "small_rows": case_small_rows(), "write_pose": case_write_pose(),
            "node_params": case_node_params()}


# ------------------------------------------------------------------------------------------------ stage 2, directed
def build_loop_world(rng, slots, params=None, capacity=None, base_capacity=None, n_readings=12, tmp_first=None,
                     per_slot=40) -> dict:
    """slots: per search slot a list of chains dict(coarse=(response, var_x, var_y), fine=response or None,
    length); the coarse batch holds every chain, ordered by slot then chain, as kl_emit_batch_device emits them.
    Slot s queries the last of its graph's per_slot scans, pool slots [s * per_slot, (s + 1) * per_slot)."""
    params = dict(DEFAULT_PARAMS if params is None else params)
    count = len(slots)
    M = sum(len(s) for s in slots)
    stride = max([len(s) for s in slots] + [1]) + 1
    pool_scans = count * per_slot
    coarse = np.zeros(M, R.KT_RESULT)
    src = np.zeros(M, R.SOURCE)
    query = np.zeros(M, np.int32)
    bb = np.zeros(M + 1, np.int32)
    bi = []
    loop_chains = np.zeros((count, stride), R.LOOP_CHAIN)
    fine_response = np.zeros(M)
    m = 0
    for s, chains in enumerate(slots):
        begin = 0
        for k, ch in enumerate(chains):
            resp, vx, vy = ch["coarse"]
            cov = spd(rng)
            cov[0], cov[4] = vx, vy
            coarse[m]["response"] = resp
            coarse[m]["mean"] = rng.normal(size=3)
            coarse[m]["covariance"] = cov
            src[m] = (s, k)
            query[m] = s * per_slot + per_slot - 1
            n = int(ch.get("length", 3))
            loop_chains[s, k] = (begin, n, begin + n + 1, 0)
            bi.extend(s * per_slot + begin + i for i in range(n))
            begin += n + 2
            bb[m + 1] = len(bi)
            fine_response[m] = math.nan if ch.get("fine") is None else ch["fine"]
            m += 1
    ranges = rng.uniform(0.5, 9.0, (pool_scans + (capacity or M) + 2, n_readings))
    return dict(count=count, coarse=coarse, source=src, query=query, base_begin=bb, base_index=np.array(bi, np.int32),
                loop_chains=loop_chains, pool_ranges=ranges, pool_scans=len(ranges), fine_response=fine_response,
                fine_given=np.array([ch.get("fine") is not None for s in slots for ch in s]),
                capacity=M if capacity is None else capacity, base_capacity=len(bi) if base_capacity is None else base_capacity,
                tmp_first=pool_scans if tmp_first is None else tmp_first, params=params, n_readings=n_readings)


def fine_results(rng, lw: dict, fine_of, n_fine: int) -> np.ndarray:
    """The synthetic fine matches of the kept coarse matches: the chain's fine response (NaN where none was given)."""
    fine = np.zeros(max(len(fine_of), 1), R.KT_RESULT)
    for f in range(n_fine):
        fine[f]["response"] = lw["fine_response"][fine_of[f]]
        fine[f]["mean"] = rng.normal(size=3)
        fine[f]["covariance"] = spd(rng)
    return fine


OK_C = (0.9, 0.01, 0.02)


def loop_cases() -> dict:
    p = DEFAULT_PARAMS
    mv, mc, mf = p["loop_match_maximum_variance_coarse"], p["loop_match_minimum_response_coarse"], p["loop_match_minimum_response_fine"]
    below = np.nextafter(mv, 0.0)
    out = {}
    rng = np.random.default_rng(31)
    # the coarse test, each clause at its edge; every chain's fine match would pass
    out["coarse_edges"] = build_loop_world(rng, [
        [dict(coarse=(0.9, mv, 0.01), fine=0.9), dict(coarse=(0.9, 0.01, mv), fine=0.9), dict(coarse=(mc, 0.01, 0.01), fine=0.9),
         dict(coarse=(math.nan, 0.01, 0.01), fine=0.9), dict(coarse=(0.9, math.nan, 0.01), fine=0.9),
         dict(coarse=(np.nextafter(mc, 1.0), below, below), fine=0.9)],
        [dict(coarse=OK_C, fine=0.9)], [], [dict(coarse=(0.1, 0.01, 0.01), fine=0.9)]])
    # the fine test: < rejects, so the minimum itself and NaN are accepted; the first accepted chain wins
    out["fine_edges"] = build_loop_world(rng, [
        [dict(coarse=OK_C, fine=math.nan), dict(coarse=OK_C, fine=0.99)],
        [dict(coarse=OK_C, fine=np.nextafter(mf, 0.0)), dict(coarse=OK_C, fine=mf), dict(coarse=OK_C, fine=0.99)],
        [dict(coarse=OK_C, fine=0.2), dict(coarse=(0.2, 0.01, 0.01), fine=0.99), dict(coarse=OK_C, fine=0.2)],
        [dict(coarse=(0.2, 0.01, 0.01), fine=0.99), dict(coarse=OK_C, fine=0.3), dict(coarse=OK_C, fine=0.85, length=7),
         dict(coarse=OK_C, fine=0.95)]])
    # more accepted matches than capacity, and more base scans than base_capacity
    slots = [[dict(coarse=OK_C, fine=0.9, length=2 + (k + s) % 3) for k in range(4)] for s in range(3)]
    out["overflow"] = build_loop_world(rng, slots, capacity=7)
    out["base_overflow"] = build_loop_world(rng, slots, base_capacity=11)
    out["zero_capacity"] = build_loop_world(rng, slots, capacity=0)
    return out


# ------------------------------------------------------------------------------------------------ random
def random_world(seed: int, n_jobs=None) -> dict:
    """A stage-1 world of a few jobs whose rare exits (exact origin poses, headings beyond 2 pi, singular covariances,
    responses at the threshold, first scans, 64 and 65 links) are each drawn with a small probability."""
    rng = np.random.default_rng(1000 + seed)
    params = dict(DEFAULT_PARAMS if seed % 3 else NODE_PARAMS)
    thr = threshold(params)
    J = int(rng.integers(1, 6)) if n_jobs is None else n_jobs
    specs = []
    for _ in range(J):
        u = rng.random()
        if u < 0.03:
            s = links_spec(rng, int(rng.choice([64, 65, 66])), S=12)
        else:
            S = int(rng.integers(3, 12))
            s = spec(rng, S=S, prev=rng.random() > 0.08, running=None if rng.random() < 0.2 else (int(rng.integers(0, S - 1)), int(rng.random() < 0.7)),
                     n_near=int(rng.choice([0, 0, 1, 2, 3, 8])))
        S = len(s["poses"])
        if rng.random() < 0.15:
            s["poses"][:, 2] *= rng.choice([5.0, -9.0, 30.0])
        if rng.random() < 0.1:
            s["poses"][int(rng.integers(0, S - 1))] = [0.0, 0.0, 0.0 if rng.random() < 0.5 else rng.normal()]
        if rng.random() < 0.04:
            s["rcov"] = SINGULAR_COV if rng.random() < 0.5 else NAN_COV
        for e in s["near"]:
            v = 1.0 if u < 0.03 else rng.random()  # a job drawn for its link count keeps it
            if v < 0.25:
                e["response"] = rng.uniform(0.0, 1.0)
            elif v < 0.29:
                e["response"] = rng.choice([thr, np.nextafter(thr, math.inf), np.nextafter(thr, -math.inf)])
            if rng.random() < 0.03:
                e["cov"] = SINGULAR_COV if rng.random() < 0.5 else NAN_COV
            if u >= 0.03 and rng.random() < 0.2:
                e["linked"] = False
            if rng.random() < 0.1:
                e["mean"][2] += rng.choice([7.0, -8.0, 26.0])
        specs.append(s)
    return build_world(specs, params, flags=R.KE_WRITE_POSE if seed % 2 else 0)


def random_loop_world(seed: int) -> dict:
    rng = np.random.default_rng(5000 + seed)
    p = dict(DEFAULT_PARAMS if seed % 3 else NODE_PARAMS)
    mv, mf = p["loop_match_maximum_variance_coarse"], p["loop_match_minimum_response_fine"]

    def chain():
        resp = rng.uniform(0.0, 1.0) if rng.random() < 0.5 else 0.97
        vx, vy = (mv * rng.uniform(0.0, 1.3) if rng.random() < 0.3 else 0.001 for _ in range(2))
        if rng.random() < 0.03:
            vx = mv
        fine = rng.choice([0.2, 0.97, mf, math.nan, rng.uniform(0.0, 1.0)], p=[0.35, 0.35, 0.05, 0.05, 0.2])
        return dict(coarse=(resp, vx, vy), fine=float(fine), length=int(rng.integers(1, 6)))

    slots = [[chain() for _ in range(int(rng.choice([0, 1, 2, 3, 5])))] for _ in range(int(rng.integers(1, 6)))]
    M = sum(len(s) for s in slots)
    cap = int(rng.integers(0, M + 2)) if rng.random() < 0.2 else M + 1
    lw = build_loop_world(rng, slots, p, capacity=cap)
    lw["fine_given"][:] = True
    return lw


# ------------------------------------------------------------------------------------------------ the exits met
def stage1_exits(w: dict, links, out) -> set:
    """Which of the listed exits a world's results show, read from the inputs and the results."""
    met = set()
    thr = threshold(w["params"])
    for j, job in enumerate(w["jobs"]):
        o = out[j]
        if o["status"] == R.KE_ERANGE:
            met.add("erange")
            continue
        if o["status"] == R.KE_EINVAL:
            continue
        met.add("prev_none" if job["prev"] < 0 else "prev")
        if o["status"] == R.KE_SINGULAR:
            met.add("mean_singular")
        if o["n_links"] in (0, 1, 64):
            met.add(f"links_{o['n_links']}")
        for m in range(job["near_first"], job["near_first"] + job["near_count"]):
            r = w["near"][m]["response"]
            if r == thr:
                met.add("at_threshold")
            if r == np.nextafter(thr, math.inf):
                met.add("ulp_above_threshold")
            if r > thr and np.isnan(w["near"][m]["covariance"]).any():
                met.add("nan_covariance")
        for l in links[j, :o["n_links"]]:
            p1 = w["pool_poses"][job["pool_offset"] + l["from"]]
            if l["status"] == R.KE_SINGULAR:
                met.add("link_singular")
                continue
            if p1[0] == 0.0 and p1[1] == 0.0:
                met.add("pose1_origin" if p1[2] == 0.0 else "pose1_origin_position")
            else:
                met.add("pose1_general")
            c = R.cos(-p1[2])
            if (1.0 - c) + c != 1.0:
                met.add("one_minus_c")
            if l["kind"] in (R.KE_PREV, R.KE_RUNNING):
                h = w["pool_poses"][job["pool_offset"] + job["scan"]][2] + (0.0 - p1[2])
                if abs(h) > 6.28318530717958647692:
                    met.add("normalize_cast")
    return met


STAGE1_EXITS = {"erange", "prev_none", "prev", "mean_singular", "links_0", "links_1", "links_64", "at_threshold",
                "ulp_above_threshold", "nan_covariance", "link_singular", "pose1_origin", "pose1_origin_position",
                "pose1_general", "one_minus_c", "normalize_cast"}


def loop_exits(lw: dict, co: dict, closures) -> set:
    met = set()
    p = lw["params"]
    if co["info"][1] & R.KE_LOOP_OVERFLOW:
        met.add("coarse_overflow")
    for r in lw["coarse"]:
        if r["covariance"][0] == p["loop_match_maximum_variance_coarse"] and r["response"] > p["loop_match_minimum_response_coarse"]:
            met.add("variance_at_maximum")
    first_rejected = {}
    for f in range(co["n_fine"]):
        m = co["fine_of"][f]
        s = int(lw["source"][m]["slot"])
        resp = lw["fine_response"][m]
        if closures[s]["fine"] == f:
            if np.isnan(resp):
                met.add("nan_fine_accepted")
            if first_rejected.get(s):
                met.add("rejected_then_accepted")
        elif closures[s]["fine"] < 0 or f < closures[s]["fine"]:
            first_rejected[s] = True
    for c in closures:
        met.add("closure" if c["chain"] >= 0 else "no_closure")
    return met


LOOP_EXITS = {"coarse_overflow", "variance_at_maximum", "nan_fine_accepted", "rejected_then_accepted", "closure", "no_closure"}
