"""Plain statement of one Gauss-Newton step of the Hector scan matcher -- TEST INFRASTRUCTURE ONLY.

numpy only (float64 unless a dtype is passed), vectorised, written from the mathematics of the method
(Kohlbrecher et al., "A Flexible and Scalable SLAM System with Full 3D Motion Estimation", SSRR 2011, eq. 4-13),
not from oracle/hector_oracle.c's statement order.  It needs neither the oracle nor mpmath, so GPU-side tests can
import it too.

The map M is a grid of log-odds l; the occupancy of a cell is p = 1 - 1 / (1 + exp(l)).  M(x, y) at a
continuous map coordinate is the bilinear interpolation of the four cells around it, and grad M its exact
gradient.  For the pose xi = (tx, ty, theta) in map coordinates and the scan points s_i, with

    S_i(xi)   = R(theta) s_i + (tx, ty)
    dS_i/dxi  = [ 1 0 -sin(theta) sx - cos(theta) sy ;  0 1 cos(theta) sx - sin(theta) sy ]
    J_i       = grad M(S_i) dS_i/dxi                    (a 3-vector: gx, gy, rot)
    H         = sum_i J_i^T J_i,      b = sum_i J_i^T (1 - M(S_i))

one step is xi += H^-1 b, the rotation part cut to +-0.2 rad, and no step at all unless H00 != 0 and H11 != 0.
A point outside 0 <= x <= sx - 2, 0 <= y <= sy - 2 contributes nothing.

The tolerance of the comparison (bar) is derived here as well, from the number formats alone:

    bar_k = (n + 16) * 2^-24 * sum_i |t_ik|  +  4 * sum_i |t32_ik - t64_ik|

  * a float32 sum of n terms in any order is within (n - 1) * 2^-24 * sum |t_i| of the exact sum (Higham,
    Accuracy and Stability of Numerical Algorithms, eq. 4.4, first order); + 16 leaves room for the second-order
    part and for the final roundings;
  * t32 is the same formula evaluated in numpy float32 in the float64 evaluation's cell: |t32 - t64| is the float32
    evaluation noise of one term.  It is summed without cancellation, and the factor 4 covers an evaluation in
    another operation order and a 1-ulp difference of sin / cos / exp.
  * gx / gy are discontinuous where a coordinate crosses an integer (another cell) or the map limit.  A float32
    evaluation places a point within EPS = 2^-12 cell of its float64 coordinate (coordinates stay below 2^11
    cells in every map of the tests: 2^-13 is one float32 ulp there, and the coordinate is the sum of three rounded
    products).  A point that close to an integer or to a limit is evaluated at the four corners (x +- EPS,
    y +- EPS) as well, each corner in its own cell, and contributes the interval [min, max] of the five values.
    The compared sum then has to lie in [sum lo - bar, sum hi + bar].
"""
from __future__ import annotations

from dataclasses import dataclass

import numpy as np

EPS = 2.0 ** -12
U32 = 2.0 ** -24
CLAMP = 0.2
# the nine sums, in the order used by every [.., 9] array here
TERMS = ("b0", "b1", "b2", "H00", "H11", "H22", "H01", "H02", "H12")


@dataclass(frozen=True)
class Level:
    """One level of the map pyramid: sx x sy cells of cell_len metres; the world origin lies at map coordinate
    off / cell_len; points (given in level-0 cells) are scaled by f."""
    sx: int
    sy: int
    cell_len: float
    off: tuple
    f: float


def pyramid(map_resolution, size_x, size_y, start, levels):
    """The levels of a map of size_x x size_y cells whose world origin sits at the fraction `start` of its extent;
    every coarser level halves the cell count and doubles the cell length.  The parameters are the float32 values
    a float32 interface is given (resolution, and the offset = resolution * size * start)."""
    f32 = np.float32
    res = f32(map_resolution)
    off = (float(res * f32(size_x) * f32(start[0])), float(res * f32(size_y) * f32(start[1])))
    out = []
    for i in range(levels):
        out.append(Level(size_x >> i, size_y >> i, float(res) * 2.0 ** i, off, 2.0 ** -i))
    return out


def occupancy(l, dtype=np.float64):
    l = np.asarray(l, dtype)
    one = dtype(1.0)
    return one - one / (one + np.exp(l))


def normalize_angle(a):
    """The angle in (-pi, pi]."""
    a = float(a)
    if not np.isfinite(a):
        return a
    r = a - 2.0 * np.pi * np.floor(a / (2.0 * np.pi))   # [0, 2 pi)
    return r - 2.0 * np.pi if r > np.pi else r


def map_from_world(L: Level, w):
    w = np.asarray(w, np.float64)
    return np.array([(w[0] + L.off[0]) / L.cell_len, (w[1] + L.off[1]) / L.cell_len, w[2]])


def world_from_map(L: Level, m):
    m = np.asarray(m, np.float64)
    return np.array([m[0] * L.cell_len - L.off[0], m[1] * L.cell_len - L.off[1], m[2]])


def scan_in_map(L: Level, pose, pts, dtype=np.float64):
    """S_i(xi): the map coordinates of the scan points (pts in level-0 cells) and the scaled points."""
    p = np.asarray(pts, np.float32).reshape(-1, 2).astype(dtype) * dtype(L.f)
    tx, ty, th = (dtype(v) for v in pose)
    c, s = np.cos(th), np.sin(th)
    x = c * p[:, 0] - s * p[:, 1] + tx
    y = s * p[:, 0] + c * p[:, 1] + ty
    return x, y, p


def terms_at(L: Level, logodds, pose, p, x, y, dtype=np.float64, cell=None):
    """The nine per-point terms [n, 9] (order TERMS) of the points p (scaled) sitting at map coordinates (x, y).
    cell = (ix, iy, inside) of another evaluation fixes the cells (for the float32 noise term); returns
    (terms, (ix, iy, inside))."""
    M = np.asarray(logodds, np.float32).reshape(L.sy, L.sx)
    x = np.asarray(x, dtype)
    y = np.asarray(y, dtype)
    if cell is None:
        with np.errstate(invalid="ignore"):
            inside = (x >= 0) & (x <= L.sx - 2) & (y >= 0) & (y <= L.sy - 2)
        ix = np.where(inside, np.floor(np.where(inside, x, 0)), 0).astype(np.int64)
        iy = np.where(inside, np.floor(np.where(inside, y, 0)), 0).astype(np.int64)
    else:
        ix, iy, inside = cell
    u = (x - ix.astype(dtype)).astype(dtype)
    v = (y - iy.astype(dtype)).astype(dtype)
    one = dtype(1.0)
    p00 = occupancy(M[iy, ix], dtype)
    p10 = occupancy(M[iy, ix + 1], dtype)
    p01 = occupancy(M[iy + 1, ix], dtype)
    p11 = occupancy(M[iy + 1, ix + 1], dtype)
    val = (one - v) * ((one - u) * p00 + u * p10) + v * ((one - u) * p01 + u * p11)
    gx = (one - v) * (p10 - p00) + v * (p11 - p01)
    gy = (one - u) * (p01 - p00) + u * (p11 - p10)
    th = dtype(pose[2])
    c, s = np.cos(th), np.sin(th)
    rot = (-s * p[:, 0] - c * p[:, 1]) * gx + (c * p[:, 0] - s * p[:, 1]) * gy
    r = one - val
    t = np.stack([gx * r, gy * r, rot * r, gx * gx, gy * gy, rot * rot, gx * gy, gx * rot, gy * rot], axis=1)
    t = np.where(inside[:, None], t, dtype(0.0)).astype(dtype)
    return t, (ix, iy, inside)


@dataclass
class StepSums:
    lo: np.ndarray        # [9] sum of the per-point lower ends
    hi: np.ndarray        # [9] sum of the per-point upper ends
    bar: np.ndarray       # [9]
    n_in: int             # points inside the map (float64 evaluation)
    n_interval: int       # of them, points that took the interval branch
    terms: np.ndarray     # [n, 9] float64 terms at the points' own coordinates


def step_sums(L: Level, logodds, pose, pts) -> StepSums:
    """H and b of one step as intervals [lo, hi] with their bar (module docstring)."""
    n = int(np.asarray(pts).reshape(-1, 2).shape[0])
    x, y, p = scan_in_map(L, pose, pts)
    t64, cell = terms_at(L, logodds, pose, p, x, y)
    x32, y32, p32 = scan_in_map(L, pose, pts, np.float32)
    t32, _ = terms_at(L, logodds, pose, p32, x32, y32, np.float32, cell=cell)
    noise = np.abs(t32.astype(np.float64) - t64)
    lo = t64.copy()
    hi = t64.copy()

    def near(a):   # of an integer: a cell border, or a map limit (0 and size - 2 are integers too)
        return np.abs(a - np.round(a)) <= EPS

    with np.errstate(invalid="ignore"):
        close = (x >= -EPS) & (x <= L.sx - 2 + EPS) & (y >= -EPS) & (y <= L.sy - 2 + EPS)
        iv = close & (near(x) | near(y))
    k = np.flatnonzero(iv)
    if k.size:
        for dx in (-EPS, EPS):
            for dy in (-EPS, EPS):
                tc, ccell = terms_at(L, logodds, pose, p[k], x[k] + dx, y[k] + dy)
                lo[k] = np.minimum(lo[k], tc)
                hi[k] = np.maximum(hi[k], tc)
                # the float32 noise of the corner's own cell
                tc32, _ = terms_at(L, logodds, pose, p32[k], (x[k] + dx).astype(np.float32),
                                   (y[k] + dy).astype(np.float32), np.float32, cell=ccell)
                noise[k] = np.maximum(noise[k], np.abs(tc32.astype(np.float64) - tc))
    mag = np.maximum(np.abs(lo), np.abs(hi)).sum(axis=0)
    bar = (n + 16) * U32 * mag + 4.0 * noise.sum(axis=0)
    inside = cell[2]
    return StepSums(lo.sum(axis=0), hi.sum(axis=0), bar, int(inside.sum()), int(iv.sum()), t64)


def assemble(s9):
    """(H [3, 3], b [3]) from nine sums in the order TERMS."""
    b0, b1, b2, h00, h11, h22, h01, h02, h12 = (float(v) for v in s9)
    return np.array([[h00, h01, h02], [h01, h11, h12], [h02, h12, h22]]), np.array([b0, b1, b2])


def sums_of_trace_row(row):
    """The nine sums (order TERMS) of one HectorOracle.trace() row: pose[3], H[9] row-major, b[3]."""
    r = np.asarray(row, np.float64)
    H = r[3:12].reshape(3, 3)
    return np.array([r[12], r[13], r[14], H[0, 0], H[1, 1], H[2, 2], H[0, 1], H[0, 2], H[1, 2]])


def solve_step(H, b):
    """The pose change of one step: (d [3], updated, clamped).  No update unless H00 != 0 and H11 != 0; the
    rotation part is cut to +-CLAMP (float32(0.2), the constant a float32 implementation compares with)."""
    H = np.asarray(H, np.float64)
    b = np.asarray(b, np.float64)
    if H[0, 0] == 0.0 or H[1, 1] == 0.0:
        return np.zeros(3), False, 0
    try:
        d = np.linalg.solve(H, b)
    except np.linalg.LinAlgError:
        return np.full(3, np.nan), True, 0
    lim = float(np.float32(CLAMP))
    clamped = 0
    if d[2] > lim:
        d[2], clamped = lim, 1
    elif d[2] < -lim:
        d[2], clamped = -lim, -1
    return d, True, clamped


def gn_step(L: Level, logodds, pose, pts):
    """One whole step from the map: the new pose (float64), H, b, updated, clamped."""
    t, _ = terms_at(L, logodds, pose, *_swap(scan_in_map(L, pose, pts)))
    H, b = assemble(np.sum(t, axis=0))
    d, upd, cl = solve_step(H, b)
    return np.asarray(pose, np.float64) + d, H, b, upd, cl


def _swap(xyp):
    x, y, p = xyp
    return p, x, y


def steps_per_level(levels):
    """Gauss-Newton steps of a match, finest level last: 1 + 5 on level 0, 1 + 3 on every coarser one."""
    return [6 if lvl == 0 else 4 for lvl in range(levels - 1, -1, -1)]
