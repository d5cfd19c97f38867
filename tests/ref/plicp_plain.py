"""A plain reference for ONE iteration of point-to-line ICP (A. Censi, "An ICP variant using a point-to-line
metric", ICRA 2008; the loop oracle/plicp_oracle.c's header describes), written from the algorithm and not
from the kernel: libm atan / atan2 / sin / cos, numpy argmin and sort, the point-to-segment distance as a
clamped projection, and the estimate (the sums M = sum M_k^T C M_k, g = -2 sum M_k^T C q, the Schur
complement, the Lagrange multiplier by root finding and the back-substitution) in mpmath at 50 digits.
Neither the kernel's operation order nor its deterministic math (detmath.h) appears here, so what this file
and oracle/plicp_oracle.c agree on is pinned by two independent statements of the published algorithm.

    step(ref_r, sens_r, theta, x_old, params) -> dict(status, x_new, nvalid, error, kept)

tests/ref/make_plicp_golden.py stores its results (tests/golden/plicp_plain_steps.npz);
tests/test_plicp_cpu.py holds the oracle to them and tests/test_plicp_gpu.py the kernel.
"""
import math

import numpy as np

PARAM_NAMES = ("max_angular_correction_deg", "max_linear_correction", "epsilon_xy", "epsilon_theta",
               "max_correspondence_dist", "outliers_maxPerc", "outliers_adaptive_order", "outliers_adaptive_mult",
               "max_iterations", "use_point_to_line_distance", "outliers_remove_doubles")
# ScanMatchPLICP::InitParams (lesson3/src/plicp_odometry.cc:74-186)
DEFAULTS = dict(max_angular_correction_deg=45.0, max_linear_correction=1.0, epsilon_xy=1e-6, epsilon_theta=1e-6,
                max_correspondence_dist=1.0, outliers_maxPerc=0.90, outliers_adaptive_order=0.7,
                outliers_adaptive_mult=2.0, max_iterations=10, use_point_to_line_distance=1,
                outliers_remove_doubles=1)


def cartesian(theta, r):
    """valid <=> reading > 0 (NaN is invalid); points r (cos theta, sin theta)."""
    r = np.asarray(r, np.float64)
    with np.errstate(invalid="ignore"):
        valid = r > 0.0
    rr = np.where(valid, r, 0.0)
    return valid, np.stack([rr * np.cos(theta), rr * np.sin(theta)], axis=1)


def _interval(P, w, n, min_theta, max_theta):
    """possible_interval: the rays within max_angular_correction + atan(max_linear_correction / |w|) of w's
    polar angle, as cells of the mean angular resolution."""
    angle_res = (max_theta - min_theta) / n
    norm = math.hypot(w[0], w[1])
    lin = math.atan(P["max_linear_correction"] / norm) if norm > 0.0 else math.pi / 2
    delta = abs(math.radians(P["max_angular_correction_deg"])) + abs(lin)
    rng = int(math.ceil(delta / angle_res))
    start = math.atan2(w[1], w[0])
    if start < min_theta:
        start += 2.0 * math.pi
    if start > max_theta:
        start -= 2.0 * math.pi
    cell = int((start - min_theta) / (max_theta - min_theta) * n)
    return min(max(cell - rng, 0), n - 1), min(max(cell + rng, 0), n - 1)


def _dist_to_segment(a, b, w):
    """|w - the point of segment ab closest to w|: the projection parameter clamped to [0, 1]."""
    ab = b - a
    t = float(np.dot(w - a, ab) / np.dot(ab, ab))
    q = a + min(max(t, 0.0), 1.0) * ab
    return math.hypot(w[0] - q[0], w[1] - q[1])


def correspondences(ref_r, sens_r, theta, x_old, P):
    """Search, rejection and the two outlier filters.  Returns None when fewer than 5 % of the rays found a
    correspondence, else (kept [(i, j1, j2)], nvalid, error, ref points, sensor points)."""
    theta = np.asarray(theta, np.float64)
    n = theta.shape[0]
    rv, rp = cartesian(theta, ref_r)
    sv, sp = cartesian(theta, sens_r)
    c, s = math.cos(x_old[2]), math.sin(x_old[2])
    W = sp @ np.array([[c, s], [-s, c]]) + np.array([x_old[0], x_old[1]])   # R(theta) p + t
    maxd2 = P["max_correspondence_dist"] ** 2
    ridx = np.flatnonzero(rv)
    corr = []   # (i, j1, j2, dist^2, e)
    for i in np.flatnonzero(sv):
        w = W[i]
        lo, hi = _interval(P, w, n, float(theta[0]), float(theta[-1]))
        cand = ridx[(ridx >= lo) & (ridx <= hi)]
        if cand.size == 0:
            continue
        d = ((rp[cand] - w) ** 2).sum(axis=1)
        k = int(np.argmin(d))
        j1, dist2 = int(cand[k]), float(d[k])
        if dist2 > maxd2 or j1 == 0 or j1 == n - 1:
            continue
        below, above = ridx[ridx < j1], ridx[ridx > j1]
        if below.size == 0 and above.size == 0:
            continue
        if above.size == 0:
            j2 = int(below[-1])
        elif below.size == 0:
            j2 = int(above[0])
        else:
            up, dn = int(above[0]), int(below[-1])
            j2 = up if ((rp[up] - w) ** 2).sum() < ((rp[dn] - w) ** 2).sum() else dn
        corr.append((int(i), j1, j2, dist2, _dist_to_segment(rp[j1], rp[j2], w)))
    if len(corr) < 0.05 * n:
        return None
    # trimming: keep e <= min(e_(k maxPerc), mult * e_(k adaptive_order)) of the k sorted errors
    e = np.sort(np.array([q[4] for q in corr]))
    k = e.shape[0]

    def stat(perc):
        return e[min(max(int(math.floor(k * perc)), 0), k - 1)]

    limit = min(stat(P["outliers_maxPerc"]), P["outliers_adaptive_mult"] * stat(P["outliers_adaptive_order"]))
    corr = [q for q in corr if q[4] <= limit]
    nvalid = len(corr)
    error = math.fsum(q[4] for q in corr)
    # doubles: of the points sharing one j1, drop those more than 3 x (9 x squared) as far as the nearest
    if P["outliers_remove_doubles"]:
        nearest = {}
        for q in corr:
            nearest[q[1]] = min(nearest.get(q[1], math.inf), q[3])
        corr = [q for q in corr if not q[3] > 9.0 * nearest[q[1]]]
    return [(q[0], q[1], q[2]) for q in corr], nvalid, error, rp, sp


def estimate(kept, rp, sp, point_to_line, digits=50):
    """argmin over (t, theta) of sum (R p + t - q)^T C (R p + t - q), C = n n^T (n the normal of the segment
    j1-j2) or I: x = (t, cos, sin), minimise x^T M x + g^T x on cos^2 + sin^2 = 1.  Returns None when the
    problem is degenerate (A singular or h = 0)."""
    import mpmath as mp

    with mp.workdps(digits):
        f = mp.mpf
        # C = sum over its rows a of a a^T (the segment's normal, or the two unit vectors for point-to-point), so
        # M_k^T C M_k = sum v v^T and M_k^T C q = sum v (a . q) with v = M_k^T a; plain mpf scalars throughout
        Ms = [[f(0)] * 4 for _ in range(4)]
        gs = [f(0)] * 4
        one, zero = f(1), f(0)
        for i, j1, j2 in kept:
            px, py = f(float(sp[i, 0])), f(float(sp[i, 1]))
            qx, qy = f(float(rp[j1, 0])), f(float(rp[j1, 1]))
            if point_to_line:
                dx, dy = qx - f(float(rp[j2, 0])), qy - f(float(rp[j2, 1]))
                ln = mp.sqrt(dx * dx + dy * dy)
                rows = ((dy / ln, -dx / ln),)
            else:
                rows = ((one, zero), (zero, one))
            for ax, ay in rows:
                # R p + t = M_k (tx, ty, cos, sin), M_k = [[1, 0, px, -py], [0, 1, py, px]]
                v = (ax, ay, ax * px + ay * py, ay * px - ax * py)
                aq = ax * qx + ay * qy
                for u in range(4):
                    for w in range(u, 4):
                        Ms[u][w] = Ms[u][w] + v[u] * v[w]
                    gs[u] = gs[u] - 2 * (v[u] * aq)
        M = mp.matrix(4, 4)
        for u in range(4):
            for w in range(4):
                M[u, w] = Ms[min(u, w)][max(u, w)]
        g = mp.matrix(gs)
        A, B, D = M[0:2, 0:2], M[0:2, 2:4], M[2:4, 2:4]
        if not mp.det(A) > 0:
            return None
        Ai = mp.inverse(A)
        S = D - B.T * Ai * B
        gt, gr = g[0:2, 0], g[2:4, 0]
        h = -gr / 2 + B.T * Ai * gt / 2
        hn = mp.norm(h)
        if not hn > 0:
            return None
        # stationarity: (S + l I) r = h with |r| = 1; the minimum has S + l I >= 0, and |(S + l I)^-1 h| falls
        # from +inf to <= 1 on (-lmin(S), -lmin(S) + |h|]: its one root there is the multiplier
        mid = (S[0, 0] + S[1, 1]) / 2
        lmin = mid - mp.sqrt(((S[0, 0] - S[1, 1]) / 2) ** 2 + S[0, 1] ** 2)

        def solve(l):
            a, d, b = S[0, 0] + l, S[1, 1] + l, S[0, 1]
            det = a * d - b * b
            return mp.matrix([(d * h[0] - b * h[1]) / det, (a * h[1] - b * h[0]) / det])

        def excess(l):   # 1 / |r(l)| - 1: rises from -1 to >= 0 over the bracket and is close to linear in l
            return 1 / mp.norm(solve(l)) - 1

        lo, hi = -lmin + hn * f(10) ** (-(digits - 5)), -lmin + hn
        if excess(hi) == 0:
            lam = hi
        else:
            lam = mp.findroot(excess, (lo, hi), solver="illinois", tol=f(10) ** (-(digits - 8)), maxsteps=400)
        # (point-to-point has S = s I and the root at hi itself, to rounding)
        assert lo <= lam <= hi + (hi - lo) * f(10) ** (-(digits - 15)) and abs(excess(lam)) < f(10) ** (-(digits - 15))
        r = solve(lam)
        t = -(Ai * (B * r + gt / 2))
        x = [float(t[0]), float(t[1]), float(mp.atan2(r[1], r[0]))]
    return x if all(math.isfinite(v) for v in x) else None


def step(ref_r, sens_r, theta, x_old, params=None):
    """One ICP iteration from x_old.  status: "ok", "few_corr" or "solve"."""
    P = dict(DEFAULTS)
    P.update(params or {})
    found = correspondences(ref_r, sens_r, theta, x_old, P)
    if found is None:
        return dict(status="few_corr", x_new=None, nvalid=0, error=0.0, kept=[])
    kept, nvalid, error, rp, sp = found
    x = estimate(kept, rp, sp, bool(P["use_point_to_line_distance"]))
    return dict(status="ok" if x is not None else "solve", x_new=x, nvalid=nvalid, error=error, kept=kept)
