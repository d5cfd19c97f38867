"""Karto's pose-graph optimiser over the MI355X C-ABI (include/slam2d/spa.h).

Reference: MapperGraph::CorrectPoses (lesson6/lib/open_karto/src/Mapper.cpp:1397-1414) -> SpaSolver::Compute
(lesson6/src/spa_solver/spa_solver.cc:43-61) -> SysSPA2d::doSPA (lesson6/lib/sparse_bundle_adjustment/src/
spa2d.cpp:425-609), run here in its block-Jacobi PCG mode (SBA_BLOCK_JACOBIAN_PCG, solver="pcg", the default) or with
a direct envelope Cholesky solve (solver="cholesky"; the node's doSPA(40) solves directly too, through CSparse /
CHOLMOD in an order of their own).  `SpaSolver` carries the reference's method names; `SpaFleet` holds a batch of
independent graphs.  Results are checked against tests/ref/spa2d_ref.c and tests/ref/spa2d_chol_ref.c (parity
unpinned against the compiled library: Eigen and SuiteSparse are absent).
"""
from __future__ import annotations

import ctypes as C
import math

import numpy as np

from . import _lib
from ._lib import Slam2dError
from ._stage import Stage, dp as _dp, hp as _hp, library

SPA_OK, SPA_EINVAL, SPA_ERANGE = 0, -1, -5
SPA_NOT_RUN, SPA_NO_FIXED, SPA_DISCONNECTED, SPA_NOT_POSDEF, SPA_FACTOR_RANGE = -100, 1, 2, 3, 4
SPA_SOLVER_PCG, SPA_SOLVER_CHOLESKY = 0, 1
SOLVERS = {"pcg": SPA_SOLVER_PCG, "cholesky": SPA_SOLVER_CHOLESKY}
SPA_FIXED_FROM_PARAMS = -2147483648
SPA_EDIT_MAX_NODES = 4096


class SpaNodeRow(C.Structure):
    _fields_ = [("graph", C.c_int), ("id", C.c_int), ("pose", C.c_double * 3)]


class SpaConRow(C.Structure):
    _fields_ = [("graph", C.c_int), ("id0", C.c_int), ("id1", C.c_int), ("pad_", C.c_int), ("mean", C.c_double * 3),
                ("prec", C.c_double * 9)]


NODE_ROW_DTYPE = np.dtype([("graph", np.int32), ("id", np.int32), ("pose", np.float64, 3)])
CON_ROW_DTYPE = np.dtype([("graph", np.int32), ("id0", np.int32), ("id1", np.int32), ("pad_", np.int32),
                          ("mean", np.float64, 3), ("prec", np.float64, 9)])


class SpaParams(C.Structure):
    _fields_ = [("niter", C.c_int), ("max_cg_iters", C.c_int), ("n_fixed", C.c_int), ("solver", C.c_int),
                ("lambda_", C.c_double), ("init_tol", C.c_double)]


class SpaStats(C.Structure):
    _fields_ = [("status", C.c_int), ("good_iter", C.c_int), ("lm_iters", C.c_int), ("rejected", C.c_int),
                ("cg_iters", C.c_int), ("converged", C.c_int), ("initial_cost", C.c_double),
                ("final_cost", C.c_double), ("lambda_", C.c_double)]

    def as_dict(self) -> dict:
        return {"status": self.status, "good_iter": self.good_iter, "lm_iters": self.lm_iters,
                "rejected": self.rejected, "cg_iters": self.cg_iters, "converged": self.converged,
                "initial_cost": self.initial_cost, "final_cost": self.final_cost, "lambda": self.lambda_}


def _declare(L):
    if getattr(L, "_spa_declared", False):
        return
    vp, i, P = C.c_void_p, C.c_int, C.POINTER
    L.spa_last_error.restype = C.c_char_p
    L.spa_version.restype = C.c_char_p
    L.spa_default_params.restype = None
    L.spa_default_params.argtypes = [P(SpaParams)]
    L.spa_create.argtypes = [P(vp), i, i, i]
    L.spa_create_ex.argtypes = [P(vp), i, i, i, i]
    L.spa_envelope_blocks.argtypes = [vp, i, i, P(C.c_longlong)]
    L.spa_destroy.argtypes = [vp]
    L.spa_add_node.argtypes = [vp, i, i, vp]
    L.spa_add_constraint.argtypes = [vp, i, i, i, vp, vp, P(i)]
    L.spa_set_graph.argtypes = [vp, i, i, vp, vp, i, vp, vp, vp]
    L.spa_clear_graph.argtypes = [vp, i]
    L.spa_set_n_fixed.argtypes = [vp, i, i]
    L.spa_get_counts.argtypes = [vp, i, P(i), P(i)]
    L.spa_compute.argtypes = [vp, i, i, P(SpaParams)]
    L.spa_compute_device.argtypes = [vp, i, i, P(SpaParams), vp]
    L.spa_compute_rows_device.argtypes = [vp, i, vp, P(SpaParams), vp]
    L.spa_export_poses_device.argtypes = [vp, i, vp, vp, vp, i, vp]
    L.spa_get_rows_info.argtypes = [vp, P(i), P(i)]
    L.spa_get_nodes.argtypes = [vp, i, vp, vp]
    L.spa_device_poses.argtypes = [vp, i, P(vp), P(i)]
    L.spa_get_stats.argtypes = [vp, i, P(SpaStats)]
    L.spa_poison_scratch.argtypes = [vp, i]
    L.spa_edit_nodes_device.argtypes = [vp, i, vp, vp, vp, vp]
    L.spa_edit_constraints_device.argtypes = [vp, i, vp, vp, vp, vp, vp]
    L.spa_get_edit_info.argtypes = [vp, P(i), P(i)]
    L.spa_download_graph.argtypes = [vp, i, P(i), P(i), P(i)] + [vp] * 10
    L._spa_declared = True


def default_params(**kw) -> SpaParams:
    """spa_default_params: niter 40, max_cg_iters 50, n_fixed 1, lambda 1e-4, init_tol 1e-8, solver "pcg"; keywords
    override (`lambda_` or `lambda` for the augmentation; solver="pcg" | "cholesky" or the SPA_SOLVER_* value)."""
    L = _lib.lib()
    _declare(L)
    p = SpaParams()
    L.spa_default_params(C.byref(p))
    for k, v in kw.items():
        k = "lambda_" if k == "lambda" else k
        if k not in ("niter", "max_cg_iters", "n_fixed", "lambda_", "init_tol", "solver"):
            raise TypeError(f"unknown parameter {k}")
        if k == "solver":
            if v not in SOLVERS and v not in SOLVERS.values():
                raise ValueError(f"solver must be one of {sorted(SOLVERS)}")
            v = SOLVERS.get(v, v)
        setattr(p, k, v)
    return p


# ------------------------------------------------------------------------------------------------ host helpers
def matrix3_inverse(m) -> np.ndarray:
    """karto::Matrix3::Inverse (lesson6/lib/open_karto/include/open_karto/Karto.h:2445-2490): InverseFast by
    cofactors, each cofactor times 1 / det.  |det| <= 1e-14 is where the reference asserts; it raises here."""
    m = np.asarray(m, np.float64).reshape(3, 3)
    k = np.empty((3, 3))
    k[0, 0] = m[1, 1] * m[2, 2] - m[1, 2] * m[2, 1]
    k[0, 1] = m[0, 2] * m[2, 1] - m[0, 1] * m[2, 2]
    k[0, 2] = m[0, 1] * m[1, 2] - m[0, 2] * m[1, 1]
    k[1, 0] = m[1, 2] * m[2, 0] - m[1, 0] * m[2, 2]
    k[1, 1] = m[0, 0] * m[2, 2] - m[0, 2] * m[2, 0]
    k[1, 2] = m[0, 2] * m[1, 0] - m[0, 0] * m[1, 2]
    k[2, 0] = m[1, 0] * m[2, 1] - m[1, 1] * m[2, 0]
    k[2, 1] = m[0, 1] * m[2, 0] - m[0, 0] * m[2, 1]
    k[2, 2] = m[0, 0] * m[1, 1] - m[0, 1] * m[1, 0]
    det = m[0, 0] * k[0, 0] + m[0, 1] * k[1, 0] + m[0, 2] * k[2, 0]
    if abs(det) <= 1e-14:
        raise Slam2dError("Matrix3::Inverse: the matrix is singular")
    return k * (1.0 / det)


def _from_axis_angle_z(radians: float) -> np.ndarray:
    """Matrix3::FromAxisAngle(0, 0, 1, radians) (Karto.h:2392-2421), term by term: [2][2] is (1 - cos) + cos."""
    c, s = math.cos(radians), math.sin(radians)
    omc = 1.0 - c
    return np.array([[0.0 * omc + c, 0.0 - s, 0.0 + 0.0], [0.0 + s, 0.0 * omc + c, 0.0 - 0.0],
                     [0.0 - 0.0, 0.0 + 0.0, 1.0 * omc + c]])


def normalize_angle(angle: float) -> float:
    """math::NormalizeAngle (open_karto/Math.h:182-211)."""
    two_pi = 2.0 * math.pi
    while angle < -math.pi:
        angle += int(angle / -two_pi) * two_pi if angle < -two_pi else two_pi
    while angle > math.pi:
        angle -= int(angle / two_pi) * two_pi if angle > two_pi else two_pi
    return angle


def _rot_pose(R, p):
    """Matrix3 * Pose2 (Karto.h:2574-2583), position rows."""
    return (R[0, 0] * p[0] + R[0, 1] * p[1] + R[0, 2] * p[2], R[1, 0] * p[0] + R[1, 1] * p[1] + R[1, 2] * p[2])


def link_info(pose1, pose2, covariance):
    """karto::LinkInfo::Update (lesson6/lib/open_karto/include/open_karto/Mapper.h:138-152): the pose difference
    Transform(pose1, Pose2()).TransformPose(pose2) (Karto.h:2870-2887, 2909-2935) and the covariance rotated by
    FromAxisAngle(0, 0, 1, -heading1), R * cov * R'.  Returns (mean[3], covariance[3, 3]), what
    spa_solver.cc:77-90 reads."""
    p1 = [float(v) for v in pose1]
    p2 = [float(v) for v in pose2]
    if p1 == [0.0, 0.0, 0.0]:  # SetTransform's rPose1 == rPose2 shortcut: identity
        R, tx, ty, th = np.eye(3), 0.0, 0.0, 0.0
    else:
        R = _from_axis_angle_z(0.0 - p1[2])
        th = 0.0 - p1[2]
        if p1[0] != 0.0 or p1[1] != 0.0:
            rx, ry = _rot_pose(R, p1)
            tx, ty = 0.0 - rx, 0.0 - ry
        else:
            tx, ty = 0.0, 0.0
    rx, ry = _rot_pose(R, p2)
    mean = np.array([tx + rx, ty + ry, normalize_angle(p2[2] + th)])
    Rc = _from_axis_angle_z(-p1[2])
    cov = np.asarray(covariance, np.float64).reshape(3, 3)
    return mean, _mul3(_mul3(Rc, cov), Rc.T)


def _mul3(a, b):
    """Matrix3 product, each element m[r][0] * n[0][c] + m[r][1] * n[1][c] + m[r][2] * n[2][c]."""
    out = np.empty((3, 3))
    for r in range(3):
        for c in range(3):
            out[r, c] = a[r, 0] * b[0, c] + a[r, 1] * b[1, c] + a[r, 2] * b[2, c]
    return out


def precision_of(covariance) -> np.ndarray:
    """The matrix SpaSolver::AddConstraint hands to addConstraint (spa_solver.cc:81-88): the inverse covariance's
    upper triangle mirrored."""
    k = matrix3_inverse(covariance)
    m = np.empty((3, 3))
    for r in range(3):
        for c in range(r, 3):
            m[r, c] = m[c, r] = k[r, c]
    return m


class SpaFleet(Stage):
    """A batch of `max_graphs` independent pose graphs, device resident; one workgroup optimises each.
    `max_factor_blocks` is the direct solve's room per graph in 3 x 3 blocks (see envelope_blocks); 0 serves the PCG
    mode only."""

    _PREFIX = "spa"

    def __init__(self, max_graphs: int, max_nodes: int, max_constraints: int, max_factor_blocks: int = 0):
        self.L = library(_declare)
        self.max_graphs, self.max_nodes, self.max_constraints = int(max_graphs), int(max_nodes), int(max_constraints)
        self.max_factor_blocks = int(max_factor_blocks)
        self.h = C.c_void_p()
        self._check(self.L.spa_create_ex(C.byref(self.h), self.max_graphs, self.max_nodes, self.max_constraints,
                                         self.max_factor_blocks), "spa_create_ex")

    def add_node(self, g: int, id_: int, pose):
        p = np.ascontiguousarray(pose, np.float64).reshape(3)
        self._check(self.L.spa_add_node(self.h, g, int(id_), _hp(p)), "spa_add_node")

    def add_constraint(self, g: int, id0: int, id1: int, mean, prec) -> bool:
        """addConstraint's bool: False when an id is unknown (nothing is added)."""
        m = np.ascontiguousarray(mean, np.float64).reshape(3)
        k = np.ascontiguousarray(prec, np.float64).reshape(9)
        added = C.c_int(0)
        self._check(self.L.spa_add_constraint(self.h, g, int(id0), int(id1), _hp(m), _hp(k), C.byref(added)),
                    "spa_add_constraint")
        return bool(added.value)

    def set_graph(self, g: int, ids, poses, ends, means, precs):
        ids = np.ascontiguousarray(ids, np.int32).reshape(-1)
        poses = np.ascontiguousarray(poses, np.float64).reshape(-1, 3)
        ends = np.ascontiguousarray(ends, np.int32).reshape(-1, 2)
        means = np.ascontiguousarray(means, np.float64).reshape(-1, 3)
        precs = np.ascontiguousarray(precs, np.float64).reshape(-1, 9)
        if len(ids) != len(poses) or not (len(ends) == len(means) == len(precs)):
            raise ValueError("the arrays disagree on the node or constraint count")
        self._check(self.L.spa_set_graph(self.h, g, len(ids), _hp(ids), _hp(poses), len(ends), _hp(ends), _hp(means),
                                         _hp(precs)), "spa_set_graph")

    def clear_graph(self, g: int):
        self._check(self.L.spa_clear_graph(self.h, g), "spa_clear_graph")

    def set_n_fixed(self, g: int, n_fixed: int | None):
        """SysSPA2d::nFixed of graph g; None goes back to the params' value."""
        self._check(self.L.spa_set_n_fixed(self.h, g, SPA_FIXED_FROM_PARAMS if n_fixed is None else int(n_fixed)),
                    "spa_set_n_fixed")

    def counts(self, g: int):
        n, m = C.c_int(0), C.c_int(0)
        self._check(self.L.spa_get_counts(self.h, g, C.byref(n), C.byref(m)), "spa_get_counts")
        return n.value, m.value

    def envelope_blocks(self, g: int, n_fixed: int = 1) -> int:
        """spa_envelope_blocks: the 3 x 3 blocks graph g's factor needs with its first n_fixed nodes fixed."""
        blocks = C.c_longlong(0)
        self._check(self.L.spa_envelope_blocks(self.h, g, int(n_fixed), C.byref(blocks)), "spa_envelope_blocks")
        return blocks.value

    def compute(self, g_first: int = 0, count: int | None = None, params: SpaParams | None = None):
        """doSPA on graphs [g_first, g_first + count), waiting for the result."""
        count = self.max_graphs - g_first if count is None else count
        p = params if params is not None else default_params()
        self._check(self.L.spa_compute(self.h, int(g_first), int(count), C.byref(p)), "spa_compute")

    def compute_device(self, g_first: int = 0, count: int | None = None, params: SpaParams | None = None,
                       hip_stream: int = 0):
        """The same, enqueued on hip_stream (0: the context's) without waiting."""
        count = self.max_graphs - g_first if count is None else count
        p = params if params is not None else default_params()
        self._check(self.L.spa_compute_device(self.h, int(g_first), int(count), C.byref(p),
                                              C.c_void_p(hip_stream or None)), "spa_compute_device")

    def compute_rows_device(self, n_rows: int, d_graph: int, params: SpaParams | None = None, hip_stream: int = 0):
        """spa_compute_rows_device: doSPA on the graphs the `n_rows` ints at device address d_graph name."""
        p = params if params is not None else default_params()
        self._check(self.L.spa_compute_rows_device(self.h, int(n_rows), _dp(d_graph), C.byref(p), _dp(hip_stream)),
                    "spa_compute_rows_device")

    def export_poses_device(self, n_rows: int, d_graph: int, d_pool_offset: int, d_pool_poses: int, pool_scans: int,
                            hip_stream: int = 0):
        """spa_export_poses_device: CorrectPoses' loop, pool[offset[g] + id] = pose for the named graphs' nodes."""
        self._check(self.L.spa_export_poses_device(self.h, int(n_rows), _dp(d_graph), _dp(d_pool_offset),
                                                   _dp(d_pool_poses), int(pool_scans), _dp(hip_stream)),
                    "spa_export_poses_device")

    def rows_info(self):
        """(rows or nodes the two row-indexed calls refused since the last call, status of the first); waits."""
        n, st = C.c_int(0), C.c_int(0)
        self._check(self.L.spa_get_rows_info(self.h, C.byref(n), C.byref(st)), "spa_get_rows_info")
        return n.value, st.value

    def get_nodes(self, g: int):
        """(ids [n], poses [n, 3]) in node order."""
        n, _ = self.counts(g)
        ids, poses = np.zeros(n, np.int32), np.zeros((n, 3), np.float64)
        self._check(self.L.spa_get_nodes(self.h, g, _hp(ids), _hp(poses)), "spa_get_nodes")
        return ids, poses

    def device_poses(self, g: int):
        """(device address of double[n][3], n): the d_poses kg_build_device and kt_set_scans_device take."""
        ptr, n = C.c_void_p(), C.c_int(0)
        self._check(self.L.spa_device_poses(self.h, g, C.byref(ptr), C.byref(n)), "spa_device_poses")
        return int(ptr.value or 0), n.value

    def stats(self, g: int) -> dict:
        st = SpaStats()
        self._check(self.L.spa_get_stats(self.h, g, C.byref(st)), "spa_get_stats")
        return st.as_dict()

    def poison_scratch(self, byte: int = 0xFF):
        self._check(self.L.spa_poison_scratch(self.h, int(byte)), "spa_poison_scratch")

    # ------------------------------------------------------------------------------------------------ device edits
    def edit_nodes_device(self, count: int, d_rows: int, d_mask: int = 0, d_status: int = 0, hip_stream: int = 0):
        """spa_edit_nodes_device: `count` spa_node_row rows (NODE_ROW_DTYPE) at device address d_rows."""
        self._check(self.L.spa_edit_nodes_device(self.h, int(count), _dp(d_rows), _dp(d_mask), _dp(d_status),
                                                 _dp(hip_stream)), "spa_edit_nodes_device")

    def edit_constraints_device(self, count: int, d_rows: int, d_mask: int = 0, d_added: int = 0, d_status: int = 0,
                                hip_stream: int = 0):
        """spa_edit_constraints_device: `count` spa_con_row rows (CON_ROW_DTYPE) at device address d_rows."""
        self._check(self.L.spa_edit_constraints_device(self.h, int(count), _dp(d_rows), _dp(d_mask), _dp(d_added),
                                                       _dp(d_status), _dp(hip_stream)), "spa_edit_constraints_device")

    def edit_info(self):
        """(rows refused since the last call, status of the first); waits."""
        n, st = C.c_int(0), C.c_int(0)
        self._check(self.L.spa_get_edit_info(self.h, C.byref(n), C.byref(st)), "spa_get_edit_info")
        return n.value, st.value

    def download_graph(self, g: int) -> dict:
        """Graph g's DEVICE arrays (pending host edits are uploaded first): ids, ends, means, precs and the six
        index lists, each cut to its length."""
        n, m, p = C.c_int(0), C.c_int(0), C.c_int(0)
        nul = [None] * 10
        self._check(self.L.spa_download_graph(self.h, g, C.byref(n), C.byref(m), C.byref(p), *nul), "spa_download_graph")
        n, m, p = n.value, m.value, p.value
        out = {"ids": np.zeros(n, np.int32), "ends": np.zeros((m, 2), np.int32), "means": np.zeros((m, 3)),
               "precs": np.zeros((m, 9)), "inc_off": np.zeros(n + 1, np.int32), "inc": np.zeros(2 * m, np.int32),
               "nbr_off": np.zeros(n + 1, np.int32), "nbr": np.zeros((2 * m, 2), np.int32),
               "pair_off": np.zeros(p + 1, np.int32), "pair_con": np.zeros(m, np.int32)}
        self._check(self.L.spa_download_graph(self.h, g, None, None, None, *[_hp(a) for a in out.values()]),
                    "spa_download_graph")
        out["nbr"] = out["nbr"][:int(out["nbr_off"][n])].copy()
        out.update(n_nodes=n, n_cons=m, n_pairs=p)
        return out


class SpaSolver:
    """lesson6's SpaSolver (spa_solver.cc:32-91) over one device graph: AddNode, AddConstraint, Compute,
    GetCorrections, Clear.  solver="cholesky" selects the direct solve, with factor storage for the full triangle of
    max_nodes; `params`, when given, is used as it is and its solver field must agree."""

    def __init__(self, max_nodes: int = 2048, max_constraints: int = 8192, params: SpaParams | None = None,
                 solver: str = "pcg"):
        if solver not in SOLVERS:
            raise ValueError(f"solver must be one of {sorted(SOLVERS)}")
        self.params = params if params is not None else default_params(solver=solver)
        if self.params.solver != SOLVERS[solver]:
            raise ValueError("params.solver and solver disagree")
        blocks = max_nodes * (max_nodes + 1) // 2 if solver == "cholesky" else 0
        self.fleet = SpaFleet(1, max_nodes, max_constraints, blocks)
        self.corrections: list = []

    def close(self):
        self.fleet.close()

    def Clear(self):
        """spa_solver.cc:32-35: only the corrections; m_Spa keeps its nodes and constraints."""
        self.corrections = []

    def GetCorrections(self) -> list:
        return self.corrections

    def AddNode(self, unique_id: int, corrected_pose):
        """spa_solver.cc:63-68: the vertex's corrected pose (x, y, heading) under its unique id."""
        self.fleet.add_node(0, unique_id, corrected_pose)

    def AddConstraint(self, source_id: int, target_id: int, pose_difference, covariance) -> bool:
        """spa_solver.cc:70-91: the link's pose difference and the inverse of its covariance (link_info() makes
        both from two poses and a covariance, as LinkInfo::Update does)."""
        return self.fleet.add_constraint(0, source_id, target_id, pose_difference, precision_of(covariance))

    def Compute(self) -> list:
        """spa_solver.cc:43-61: doSPA, then (id, pose) for every node."""
        self.corrections = []
        self.fleet.compute(0, 1, self.params)
        ids, poses = self.fleet.get_nodes(0)
        self.corrections = [(int(i), p.copy()) for i, p in zip(ids, poses)]
        return self.corrections

    def stats(self) -> dict:
        return self.fleet.stats(0)
