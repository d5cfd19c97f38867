"""Plain numpy float64 Levenberg-Marquardt for the pose-graph cost SysSPA2d minimises, solving every step exactly.

The method without any of this project's choices: no block-Jacobi PCG, no fixed summation order, numpy's cos / sin,
a dense normal-equation matrix and numpy.linalg.solve.  What it shares with doSPA (spa2d.cpp:425-609) is the
problem: the error h(x) - z of calcErr (:148-159) with its +-pi wrap, the cost sum of err' * prec * err, the
diagonal scaled by 1 + lambda, the accept (lambda / 2) or undo (lambda * laminc, laminc * 2) rule, and the
squared-step convergence test.  Test infrastructure only.
"""
from __future__ import annotations

import math

import numpy as np


def _err(p0, p1, mean):
    c, s = math.cos(p0[2]), math.sin(p0[2])
    dx, dy = p1[0] - p0[0], p1[1] - p0[1]
    a = (p1[2] - p0[2]) - mean[2]
    if a > math.pi:
        a -= 2.0 * math.pi
    if a < -math.pi:
        a += 2.0 * math.pi
    return np.array([c * dx + s * dy - mean[0], -s * dx + c * dy - mean[1], a])


def cost(poses, ends, means, precs) -> float:
    total = 0.0
    for (a, b), z, k in zip(ends, means, precs):
        e = _err(poses[a], poses[b], z)
        total += float(e @ k.reshape(3, 3) @ e)
    return total


def _jacobians(p0, p1):
    c, s = math.cos(p0[2]), math.sin(p0[2])
    dx, dy = p1[0] - p0[0], p1[1] - p0[1]
    j0 = np.array([[-c, -s, -s * dx + c * dy], [s, -c, -c * dx - s * dy], [0.0, 0.0, -1.0]])
    j1 = np.array([[c, s, 0.0], [-s, c, 0.0], [0.0, 0.0, 1.0]])
    return j0, j1


def solve(poses, ends, means, precs, n_fixed=1, niter=40, lam=1e-4, sq_min_delta=1e-16):
    """(poses_out, stats): LM with exact steps from the same start."""
    poses = np.array(poses, np.float64).reshape(-1, 3).copy()
    ends = np.asarray(ends).reshape(-1, 2)
    means = np.asarray(means, np.float64).reshape(-1, 3)
    precs = np.asarray(precs, np.float64).reshape(-1, 9)
    n = len(poses)
    nfree = n - n_fixed
    laminc = 2.0
    c0 = cur = cost(poses, ends, means, precs)
    st = {"lm_iters": 0, "good_iter": 0, "rejected": 0, "converged": 0, "initial_cost": c0}
    for it in range(niter):
        st["lm_iters"] = it + 1
        H = np.zeros((3 * nfree, 3 * nfree))
        g = np.zeros(3 * nfree)
        for (a, b), z, k in zip(ends, means, precs):
            K = k.reshape(3, 3)
            e = _err(poses[a], poses[b], z)
            j0, j1 = _jacobians(poses[a], poses[b])
            ia, ib = 3 * (a - n_fixed), 3 * (b - n_fixed)
            if ia >= 0:
                H[ia:ia + 3, ia:ia + 3] += j0.T @ K @ j0
                g[ia:ia + 3] -= j0.T @ K @ e
            if ib >= 0:
                H[ib:ib + 3, ib:ib + 3] += j1.T @ K @ j1
                g[ib:ib + 3] -= j1.T @ K @ e
            if ia >= 0 and ib >= 0:
                H[ia:ia + 3, ib:ib + 3] += j0.T @ K @ j1
                H[ib:ib + 3, ia:ia + 3] += j1.T @ K @ j0
        H[np.diag_indices_from(H)] *= 1.0 + lam
        step = np.linalg.solve(H, g) if nfree > 0 else np.zeros(0)
        if float(step @ step) < sq_min_delta:
            st["converged"] = 1
            break
        old = poses.copy()
        poses[n_fixed:] += step.reshape(-1, 3)
        th = poses[n_fixed:, 2]
        th = np.where(th > math.pi, th - 2.0 * math.pi, th)
        poses[n_fixed:, 2] = np.where(th < -math.pi, th + 2.0 * math.pi, th)
        new = cost(poses, ends, means, precs)
        if new < cur:
            cur = new
            lam *= 0.5
            st["good_iter"] += 1
        else:
            lam *= laminc
            laminc *= 2.0
            poses = old
            st["rejected"] += 1
    st["final_cost"] = cur
    return poses, st
