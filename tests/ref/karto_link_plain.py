"""A literal Python transcription of the open_karto members behind the graph-linking stage, member by member, for the
tests: none of the batch or wave formulations of include/slam2d/karto_link.h appears here.

  normalize_angle                     math::NormalizeAngle, Math.h:182-210 (the (kt_int32u) casts included)
  Pose2, Matrix3                      Karto.h:2101-2141 (==, +=, +, -), :2367-2375, :2392-2493, :2552-2599
  Transform                           Karto.h:2860-2935 (SetTransform's three branches, TransformPose)
  LinkInfo                            Mapper.h:138-152
  precision_matrix                    SpaSolver::AddConstraint, spa_solver.cc:81-88
  compute_weighted_mean               Mapper.cpp:1288-1330
  MapperGraph.add_edges, link_scans,  Mapper.cpp:902-973, :1104-1167 with one sensor, the matcher's and the search's
    link_near_chains, link_chain_to_scan   results given (the world of karto_link_cases.py)
  try_close_loop                      one pass of the while loop of Mapper.cpp:986-1048, up to the first closure

sin / cos / atan2 are the restatement's exported detmath wrappers (the only arithmetic not Python's own); Python's
float is an IEEE double and its expressions are evaluated left to right without contraction.  Where the reference
asserts, Singular is raised.  Test infrastructure: nothing here is imported by the package.
"""
from __future__ import annotations

import math

import karto_link_ref as R

KT_PI = 3.14159265358979323846
KT_2PI = 6.28318530717958647692
KT_TOLERANCE = 1e-06


class Singular(Exception):
    """Matrix3::Inverse's assert(false)."""


def kt_int32u(v: float) -> int:
    return int(v) & 0xFFFFFFFF


def normalize_angle(angle: float) -> float:
    if not abs(angle) < 4294967296.0:  # the reference does not terminate: karto_link.h gives NaN
        return math.nan
    while angle < -KT_PI:
        if angle < -KT_2PI:
            angle += kt_int32u(angle / -KT_2PI) * KT_2PI
        else:
            angle += KT_2PI
    while angle > KT_PI:
        if angle > KT_2PI:
            angle -= kt_int32u(angle / KT_2PI) * KT_2PI
        else:
            angle -= KT_2PI
    return angle


class Pose2:
    def __init__(self, x=0.0, y=0.0, heading=0.0):
        self.x, self.y, self.heading = float(x), float(y), float(heading)

    def __eq__(self, o):
        return self.x == o.x and self.y == o.y and self.heading == o.heading

    def __iadd__(self, o):
        self.x += o.x
        self.y += o.y
        self.heading = normalize_angle(self.heading + o.heading)
        return self

    def __add__(self, o):
        return Pose2(self.x + o.x, self.y + o.y, normalize_angle(self.heading + o.heading))

    def __sub__(self, o):
        return Pose2(self.x - o.x, self.y - o.y, normalize_angle(self.heading - o.heading))

    def tolist(self):
        return [self.x, self.y, self.heading]


class Matrix3:
    def __init__(self, rows=None):
        self.m = [[0.0] * 3 for _ in range(3)]  # Clear()
        if rows is not None:
            flat = [float(v) for v in (rows if not hasattr(rows, "reshape") else rows.reshape(-1))]
            self.m = [flat[0:3], flat[3:6], flat[6:9]]

    def set_to_identity(self):
        self.m = [[0.0] * 3 for _ in range(3)]
        for i in range(3):
            self.m[i][i] = 1.0

    def from_axis_angle(self, x, y, z, radians):
        cosRadians = R.cos(radians)
        sinRadians = R.sin(radians)
        oneMinusCos = 1.0 - cosRadians
        xx = x * x
        yy = y * y
        zz = z * z
        xyMCos = x * y * oneMinusCos
        xzMCos = x * z * oneMinusCos
        yzMCos = y * z * oneMinusCos
        xSin = x * sinRadians
        ySin = y * sinRadians
        zSin = z * sinRadians
        m = self.m
        m[0][0] = xx * oneMinusCos + cosRadians
        m[0][1] = xyMCos - zSin
        m[0][2] = xzMCos + ySin
        m[1][0] = xyMCos + zSin
        m[1][1] = yy * oneMinusCos + cosRadians
        m[1][2] = yzMCos - xSin
        m[2][0] = xzMCos - ySin
        m[2][1] = yzMCos + xSin
        m[2][2] = zz * oneMinusCos + cosRadians

    def transpose(self):
        t = Matrix3()
        for row in range(3):
            for col in range(3):
                t.m[row][col] = self.m[col][row]
        return t

    def inverse_fast(self, inv, tolerance):
        m, i = self.m, inv.m
        i[0][0] = m[1][1] * m[2][2] - m[1][2] * m[2][1]
        i[0][1] = m[0][2] * m[2][1] - m[0][1] * m[2][2]
        i[0][2] = m[0][1] * m[1][2] - m[0][2] * m[1][1]
        i[1][0] = m[1][2] * m[2][0] - m[1][0] * m[2][2]
        i[1][1] = m[0][0] * m[2][2] - m[0][2] * m[2][0]
        i[1][2] = m[0][2] * m[1][0] - m[0][0] * m[1][2]
        i[2][0] = m[1][0] * m[2][1] - m[1][1] * m[2][0]
        i[2][1] = m[0][1] * m[2][0] - m[0][0] * m[2][1]
        i[2][2] = m[0][0] * m[1][1] - m[0][1] * m[1][0]
        fDet = m[0][0] * i[0][0] + m[0][1] * i[1][0] + m[0][2] * i[2][0]
        if abs(fDet) <= tolerance:
            return False
        if fDet != fDet:  # a NaN determinant passes the reference's test; karto_link.h refuses it
            return False
        fInvDet = 1.0 / fDet
        for row in range(3):
            for col in range(3):
                i[row][col] *= fInvDet
        return True

    def inverse(self):
        k = Matrix3([v for r in self.m for v in r])
        if not self.inverse_fast(k, 1e-14):
            raise Singular()
        return k

    def __mul__(self, o):
        if isinstance(o, Pose2):
            m = self.m
            return Pose2(m[0][0] * o.x + m[0][1] * o.y + m[0][2] * o.heading,
                         m[1][0] * o.x + m[1][1] * o.y + m[1][2] * o.heading,
                         m[2][0] * o.x + m[2][1] * o.y + m[2][2] * o.heading)
        p = Matrix3()
        for row in range(3):
            for col in range(3):
                p.m[row][col] = (self.m[row][0] * o.m[0][col] + self.m[row][1] * o.m[1][col] +
                                 self.m[row][2] * o.m[2][col])
        return p

    def __iadd__(self, o):
        for row in range(3):
            for col in range(3):
                self.m[row][col] += o.m[row][col]
        return self

    def tolist(self):
        return [v for r in self.m for v in r]


class Transform:
    def __init__(self, pose1: Pose2, pose2: Pose2):
        self.rotation, self.inverse_rotation, self.transform = Matrix3(), Matrix3(), Pose2()
        self.set_transform(pose1, pose2)

    def set_transform(self, rPose1, rPose2):
        if rPose1 == rPose2:
            self.rotation.set_to_identity()
            self.inverse_rotation.set_to_identity()
            self.transform = Pose2()
            return
        self.rotation.from_axis_angle(0, 0, 1, rPose2.heading - rPose1.heading)
        self.inverse_rotation.from_axis_angle(0, 0, 1, rPose1.heading - rPose2.heading)
        if rPose1.x != 0.0 or rPose1.y != 0.0:
            newPosition = rPose2 - self.rotation * rPose1
        else:
            newPosition = rPose2
        self.transform = Pose2(newPosition.x, newPosition.y, rPose2.heading - rPose1.heading)

    def transform_pose(self, rSourcePose):
        newPosition = self.transform + self.rotation * rSourcePose
        angle = normalize_angle(rSourcePose.heading + self.transform.heading)
        return Pose2(newPosition.x, newPosition.y, angle)


class LinkInfo:
    def __init__(self, rPose1, rPose2, rCovariance):
        self.pose1, self.pose2 = rPose1, rPose2
        transform = Transform(rPose1, Pose2())
        self.pose_difference = transform.transform_pose(rPose2)
        rotationMatrix = Matrix3()
        rotationMatrix.from_axis_angle(0, 0, 1, -rPose1.heading)
        self.covariance = rotationMatrix * rCovariance * rotationMatrix.transpose()


def precision_matrix(link: LinkInfo) -> Matrix3:
    """SpaSolver::AddConstraint's Eigen matrix m."""
    p = link.covariance.inverse()
    m = Matrix3()
    m.m[0][0] = p.m[0][0]
    m.m[0][1] = m.m[1][0] = p.m[0][1]
    m.m[0][2] = m.m[2][0] = p.m[0][2]
    m.m[1][1] = p.m[1][1]
    m.m[1][2] = m.m[2][1] = p.m[1][2]
    m.m[2][2] = p.m[2][2]
    return m


def compute_weighted_mean(rMeans, rCovariances) -> Pose2:
    assert len(rMeans) == len(rCovariances)
    inverses = []
    sumOfInverses = Matrix3()
    for cov in rCovariances:
        inverse = cov.inverse()
        inverses.append(inverse)
        sumOfInverses += inverse
    inverseOfSumOfInverses = sumOfInverses.inverse()
    accumulatedPose = Pose2()
    thetaX = 0.0
    thetaY = 0.0
    for pose, inv in zip(rMeans, inverses):
        angle = pose.heading
        thetaX += R.cos(angle)
        thetaY += R.sin(angle)
        weight = inverseOfSumOfInverses * inv
        accumulatedPose += weight * pose
    thetaX /= len(rMeans)
    thetaY /= len(rMeans)
    accumulatedPose.heading = R.atan2(thetaY, thetaX)
    return accumulatedPose


class MapperGraph:
    """AddEdges for job j of a world.  self.records collects every LinkScans call as (from, to, kind, status, diff [3],
    precision [9]): the stage emits the LinkInfo of every call, and the dedupe of AddEdge is ke_commit's."""

    def __init__(self, world: dict, j: int):
        self.w, self.job = world, world["jobs"][j]
        self.link_min = float(world["params"]["link_match_minimum_response_fine"])
        self.records = []
        self.n_means = 0
        self.mean_singular = False

    def sensor_pose(self, scan: int) -> Pose2:
        return Pose2(*self.w["pool_poses"][int(self.job["pool_offset"]) + scan])

    def link_scans(self, from_scan: int, to_scan: int, rMean: Pose2, rCovariance: Matrix3, kind: int):
        link = LinkInfo(self.sensor_pose(from_scan), rMean, rCovariance)
        try:
            prec = precision_matrix(link)
        except Singular:
            self.records.append((from_scan, to_scan, kind, R.KE_SINGULAR, [0.0] * 3, [0.0] * 9))
            return
        self.records.append((from_scan, to_scan, kind, R.KE_OK, link.pose_difference.tolist(), prec.tolist()))

    def link_chain_to_scan(self, closest: int, linked: bool, scan: int, rMean, rCovariance, kind: int):
        # GetClosestScanToPose and the distance test are the search's (kl_closest / kl_near_chain)
        if linked:
            self.link_scans(closest, scan, rMean, rCovariance, kind)

    def link_near_chains(self, scan: int, rMeans, rCovariances):
        job, w = self.job, self.w
        for k in range(int(job["near_count"])):  # the long near chains, in FindNearChains' order
            m = int(job["near_first"]) + k
            r = w["near"][m]
            mean, covariance, response = Pose2(*r["mean"]), Matrix3(r["covariance"]), float(r["response"])
            if response > self.link_min - KT_TOLERANCE:
                rMeans.append(mean)
                rCovariances.append(covariance)
                src = w["near_source"][m]
                chain = w["near_chains"][int(src["slot"]), int(src["chain"])]
                self.link_chain_to_scan(int(chain["closest"]), bool(int(chain["flags"]) & R.KL_CHAIN_LINKED), scan, mean,
                                        covariance, R.KE_NEAR)

    def add_edges(self):
        """pScan's pose after the call."""
        job = self.job
        scan, prev = int(job["scan"]), int(job["prev"])
        pose = self.sensor_pose(scan)
        means, covariances = [], []
        if prev >= 0:  # GetLastScan(rSensorName) != NULL
            rCovariance = Matrix3(self.w["seq"][int(job["seq_result"])]["covariance"])
            self.link_scans(prev, scan, pose, rCovariance, R.KE_PREV)
            scanPose = pose
            means.append(scanPose)
            covariances.append(rCovariance)
            if int(job["running"]) >= 0:
                rc = self.w["running"][int(job["running"])]
                self.link_chain_to_scan(int(rc["closest"]), bool(rc["linked"]), scan, scanPose, rCovariance, R.KE_RUNNING)
        self.link_near_chains(scan, means, covariances)
        self.n_means = len(means)
        if means:
            try:
                pose = compute_weighted_mean(means, covariances)
            except Singular:
                self.mean_singular = True
        return pose


def add_edges(world: dict):
    """Every job of a world through MapperGraph.add_edges: the (links, out, pool_poses) stage 1 must give, with POISON
    where it writes nothing.  More than max_links records is the library's KE_ERANGE."""
    jobs = world["jobs"]
    K = int(world["max_links"])
    links, out = R.poisoned((len(jobs), K), R.LINK), R.poisoned(len(jobs), R.JOB_OUT)
    pool = world["pool_poses"].copy()
    for j in range(len(jobs)):
        g = MapperGraph(world, j)
        slot = int(jobs[j]["pool_offset"]) + int(jobs[j]["scan"])
        pose = g.add_edges()
        o = out[j]
        o["graph"], o["n_links"], o["n_means"], o["status"] = jobs[j]["graph"], 0, 0, R.KE_OK
        o["pose"] = world["pool_poses"][slot]
        if len(g.records) > K:
            o["status"] = R.KE_ERANGE
            continue
        o["n_links"], o["n_means"] = len(g.records), g.n_means
        for i, (f, t, kind, st, diff, prec) in enumerate(g.records):
            links[j, i] = (f, t, kind, st, diff, prec)
        if g.mean_singular:
            o["status"] = R.KE_SINGULAR
            continue
        o["pose"] = pose.tolist()
        if int(world.get("flags", 0)) & R.KE_WRITE_POSE and g.n_means > 0:
            pool[slot] = pose.tolist()
    return links, out, pool


def try_close_loop(params: dict, chains):
    """One pass of TryCloseLoop's while loop over a slot's candidate chains, in order, up to the first closure:
    chains is a list of (coarse kt_result, fine kt_result or None).  Returns (the chains that went to the fine match,
    the index of the closing chain or -1)."""
    fine_matched, closed = [], -1
    for k, (coarse, fine) in enumerate(chains):
        coarseResponse, covariance = float(coarse["response"]), coarse["covariance"]
        if (coarseResponse > params["loop_match_minimum_response_coarse"] and
                covariance[0] < params["loop_match_maximum_variance_coarse"] and
                covariance[4] < params["loop_match_maximum_variance_coarse"]):
            fine_matched.append(k)
            if closed >= 0:
                continue  # the stage's fine batch matches every coarse-accepted chain; the first closure is kept
            fineResponse = float(fine["response"])
            if fineResponse < params["loop_match_minimum_response_fine"]:
                pass  # REJECTED!
            else:
                closed = k
    return fine_matched, closed
