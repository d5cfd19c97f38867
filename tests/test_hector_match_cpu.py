"""The Hector oracle's matcher held to the plain float64 statement of the method, step by step.

oracle/hector_oracle.c restates the reference's matcher in the kernel's float operation order, and the GPU tests
compare bits against it: an error in that restatement (a wrong interpolation weight, exchanged Hessian entries, a
wrong sign in the rotation derivative) would be copied by the kernel and pass.  Here every Gauss-Newton step the
oracle takes is compared with tests/ref/hector_match_plain.py, written from the mathematics in numpy float64:
the oracle's trace gives the map-frame pose before each step with its H and b, so each step is judged on its own
and diverging trajectories are never compared.

Bars (none is measured on the oracle):
  * H, b: hector_match_plain's bar (float32 summation bound + the float32 evaluation noise of the plain formula,
    intervals at cell borders); at most 2 % of a step's in-map points may take the interval branch.
  * the step: the oracle's own float32 H, b solved in float64; |(next - pose) - d| <= C_SOLVE cond(H) 2^-24 |d| plus
    the rounding of the float32 sum pose + d (half an ulp of either).  C_SOLVE = 8: the oracle forms the inverse from
    cofactors (two products and a difference each), a determinant of three products, a division and a 3-term
    product, about eight roundings on every path, each amplified by at most cond(H).  Steps with cond(H) > 1e5 are
    skipped (at most 10 % may be).
  * hand-off between levels, final normalize_angle, returned world pose: 2 ulp, counted at the largest magnitude
    the affine map handles (its translation term or its result) -- the float32 product and sum round there.
    Where a level ends on a step that changed the pose, the step's own tolerance is added, because the trace does
    not hold the pose after a level's last step; where it did not (H = 0), the check is the 2 ulp alone.

Measured (52 cases, 624 steps, 332 of them changing the pose): worst |oracle - plain| / bar 0.432, largest interval
share 1.49 %, 6.0 % of the steps skipped for conditioning, 62 level ends checked at 2 ulp alone.  The tests print
these figures (pytest -s); DESIGN.md section 3 records them.

The bound on the step as first written, C cond(H) 2^-24 |d| alone, cannot hold: pose + d is itself rounded to float32,
half an ulp of a coordinate of some hundred cells (3e-5) whatever |d| is, so that rounding is part of the bar.
"""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "ref"))
import hector_match_cases as K  # noqa: E402
import hector_match_plain as P  # noqa: E402
from hector_match_cases import test_case_preconditions  # noqa: E402,F401  (collected here: it needs the oracle only)

C_SOLVE = 8.0
U = 2.0 ** -24


def _ulp(v):
    return float(np.spacing(np.float32(abs(v))))


def _cases():
    out = []
    big1, big3 = K.Geo(0.05, 1024, 1024, (0.5, 0.5), 1), K.Geo(0.05, 1024, 1024, (0.5, 0.5), 3)
    hints = [(0.0, 0.0, 0.0), (0.02, -0.03, 0.01), (0.3, 0.2, 0.3), (0.0, 0.0, 0.8), (-0.1, 0.15, -0.2), (0.05, 0.0, -0.8)]
    for i, n in enumerate((1, 5, 193, 300, 577, 934)):
        for geo in (big1, big3):
            out.append(K.Case(f"big_n{n}_l{geo.levels}", geo, K.scan(0.05, n), hints[i]))
    # (a heading turned by half a circle, the runaways and the scans of 1 and 5 points are ill-conditioned: few of
    # them, so that at most 10 % of the steps are skipped)
    pick = ("small_n300_l2", "far_n300_l3", "rot08_n300_l2", "far_n1000_l4", "leave_return_n300_l2", "exact_n1000_l1",
            "heading_wrap_m_n300_l2", "heading_2pi_n300_l4", "heading_p31_n300_l2", "all_out_n300_l3",
            "all_out_far_n300_l2", "far_n1000_l2", "small_n1000_l3", "exact_n300_l4", "rot08_n1000_l3")
    by_name = {c.name: c for c in K.hint_cases()}
    out += [by_name[k] for k in pick]
    out += [c for c in K.nan_cases() if c.name != "runaway_n600_l2"] + K.clamp_cases()
    out += [c for c in K.geometry_cases() if c.name.startswith(("geo_rot", "geo_scan"))] + K.same_cell_cases()
    # hand-off alone: no point in any map (H = 0: the pose only passes through the levels' frames), assorted poses
    far = np.full((3, 2), 1.0e6, np.float32)
    for j, hint in enumerate([(1.37, -2.21, 3.3), (-0.7, 0.45, -3.4), (0.3, 0.2, 6.3), (-3.9, 2.6, -9.5), (11.0, -7.5, 1.0),
                              (0.013, 0.004, -3.1415927), (5.5, 5.5, 3.1415927)]):
        out.append(K.Case(f"handoff{j}_256", K.G256.with_levels(4), far, hint))
        out.append(K.Case(f"handoff{j}_96", K.G96, far, hint))
    names = [c.name for c in out]
    assert len(set(names)) == len(names)
    return out


@pytest.fixture(scope="module")
def runs():
    """name -> (case, pose, cov, clamps, trace) of every case in the oracle (reference summation order)."""
    return {c.name: (c,) + K.run_oracle(c, trace=True) for c in _cases()}


def _levels_of(case):
    """(level index, first trace row, rows) per level, coarsest first."""
    out, i = [], 0
    for lvl in range(case.geo.levels - 1, -1, -1):
        k = 6 if lvl == 0 else 4
        out.append((lvl, i, k))
        i += k
    return out


def test_trace_length_and_covariance(runs):
    for name, (case, pose, cov, clamps, tr) in runs.items():
        assert tr.shape[0] == sum(P.steps_per_level(case.geo.levels)), name
        np.testing.assert_array_equal(cov.view(np.int32).ravel(), tr[-1, 3:12].view(np.int32), err_msg=name)
    # an empty scan: no step at all, the hint comes back, the covariance is not written
    ora = K.G256.oracle()
    ora.enable_trace(8)
    hint = np.array([0.3, -0.2, 3.3], np.float32)
    pose, cov = ora.match(np.zeros((0, 2), np.float32), hint)
    assert ora.trace().shape[0] == 0 and not cov.any()
    np.testing.assert_array_equal(pose.view(np.int32), hint.view(np.int32))


def test_hessian_sums_against_plain(runs):
    """H and b of every step lie in the plain statement's interval, within its bar."""
    worst, worst_at, share_max, steps = 0.0, None, 0.0, 0
    for name, (case, pose, cov, clamps, tr) in runs.items():
        pyr = case.geo.pyramid()
        maps = K.maps(case.geo, case.edits)
        for lvl, first, rows in _levels_of(case):
            for i in range(first, first + rows):
                got = P.sums_of_trace_row(tr[i])
                s = P.step_sums(pyr[lvl], maps[lvl][0], tr[i, :3].astype(np.float64), case.pts)
                steps += 1
                if s.n_in:
                    share = s.n_interval / s.n_in
                    share_max = max(share_max, share)
                    assert share <= 0.02, f"{name} step {i}: {s.n_interval} of {s.n_in} points at a cell border"
                off = np.maximum(np.maximum(got - s.hi, s.lo - got), 0.0)
                with np.errstate(invalid="ignore", divide="ignore"):
                    ratio = np.where(off > 0.0, off / s.bar, 0.0)
                if ratio.max() > worst:
                    worst, worst_at = float(ratio.max()), (name, i, P.TERMS[int(ratio.argmax())])
                bad = off > s.bar
                assert not bad.any(), (f"{name} level {lvl} step {i}: " + ", ".join(
                    f"{P.TERMS[k]} oracle {got[k]:.9g} plain [{s.lo[k]:.9g}, {s.hi[k]:.9g}] bar {s.bar[k]:.3g}"
                    for k in np.flatnonzero(bad)))
    print(f"\nhessian sums: {len(runs)} cases, {steps} steps, worst |oracle - plain| / bar = {worst:.3f} at {worst_at}, "
          f"largest interval share = {100 * share_max:.2f} %")


def _handoff_tol(case, lvl_from, lvl_to, est):
    """2 ulp of the world pose at level lvl_from's frame, and of the map pose of lvl_to (None: the returned pose)."""
    pyr = case.geo.pyramid()
    A = pyr[lvl_from]
    w = P.world_from_map(A, est)
    tol_w = np.array([2 * _ulp(max(abs(A.off[k]), abs(w[k]), abs(est[k] * A.cell_len))) for k in (0, 1)] + [2 * _ulp(np.pi)])
    if lvl_to is None:
        return w, tol_w
    B = pyr[lvl_to]
    m = P.map_from_world(B, w)
    tol_m = np.array([2 * _ulp(max(abs(B.off[k] / B.cell_len), abs(m[k]))) + tol_w[k] / B.cell_len for k in (0, 1)]
                     + [2 * _ulp(np.pi)])
    return m, tol_m


def _judge(case, pose, clamps, tr):
    """One case's steps and level ends against the plain rules (asserting); returns (clamps the plain rule is sure
    of, undecided ones, updating steps, steps skipped for conditioning, level ends checked at 2 ulp alone)."""
    name = case.name
    steps = skipped = exact_handoffs = 0
    sure = unsure = 0
    levels = _levels_of(case)
    for li, (lvl, first, rows) in enumerate(levels):
        for i in range(first, first + rows):
            p0 = tr[i, :3].astype(np.float64)
            if not np.isfinite(p0).all():
                continue     # a NaN pose: every point is off the map from here on (test_hessian_sums_against_plain)
            H, b = P.assemble(P.sums_of_trace_row(tr[i]))
            d, updated, clamped = P.solve_step(H, b)
            last = i == first + rows - 1
            if last:
                lvl_to = levels[li + 1][0] if li + 1 < len(levels) else None
                got_next = (tr[i + 1, :3] if lvl_to is not None else pose).astype(np.float64)
            else:
                got_next = tr[i + 1, :3].astype(np.float64)
            if not updated:
                # the no-update rule, exactly: the pose is carried on bit for bit
                if not last:
                    np.testing.assert_array_equal(tr[i + 1, :3].view(np.int32), tr[i, :3].view(np.int32),
                                                  err_msg=f"{name} step {i}: H00 or H11 is 0, the pose must stay")
                tol_step = np.zeros(3)
                est = p0.copy()
            else:
                steps += 1
                cond = np.linalg.cond(H)
                if not np.isfinite(d).all() or not cond <= 1.0e5:
                    skipped += 1
                    unsure += 1      # nothing is claimed of an ill-conditioned step, its clamp decision included
                    continue
                raw = np.linalg.solve(H, b)
                tol_step = C_SOLVE * cond * U * np.linalg.norm(raw) + np.array([0.5 * _ulp(p0[k]) + 0.5 * _ulp(p0[k] + d[k])
                                                                                   for k in range(3)])
                if abs(abs(raw[2]) - float(np.float32(0.2))) <= tol_step[2]:
                    unsure += 1      # the rotation sits on the clamp threshold within the solve's accuracy
                    continue
                sure += abs(clamped)
                if clamped:
                    tol_step[2] = 0.5 * _ulp(p0[2]) + 0.5 * _ulp(p0[2] + d[2])   # the cut value is exact
                est = p0 + d
            if not last:
                err = np.abs(got_next - est)
                assert (err <= tol_step).all(), f"{name} step {i}: next - pose = {got_next - p0}, solve {d}, tol {tol_step}"
                continue
            # the level's end: normalize_angle, world pose, the next level's map pose (or the returned pose)
            est_n = np.array([est[0], est[1], P.normalize_angle(est[2])])
            want, tol = _handoff_tol(case, lvl, lvl_to, est_n)
            scale = case.geo.pyramid()[lvl].cell_len / (case.geo.pyramid()[lvl_to].cell_len if lvl_to is not None else 1.0)
            tol = tol + tol_step * np.array([scale, scale, 1.0])
            err = np.abs(got_next - want)
            # +-pi are one heading
            err[2] = min(err[2], abs(err[2] - 2.0 * np.pi))
            assert (err <= tol).all(), f"{name} level {lvl} end: got {got_next}, plain {want}, tol {tol}"
            assert -np.pi - 1e-6 <= got_next[2] <= np.pi + 1e-6
            exact_handoffs += not updated
    return sure, unsure, steps, skipped, exact_handoffs


def test_steps_and_handoff(runs):
    """Every step's pose change is the float64 solution of the oracle's own H and b; clamp and no-update decisions
    are the plain rule's; levels hand the pose on, and the match returns it, as the plain frames say."""
    steps = skipped = exact_handoffs = 0
    for name, (case, pose, cov, clamps, tr) in runs.items():
        sure, unsure, st, sk, ex = _judge(case, pose, clamps, tr)
        steps, skipped, exact_handoffs = steps + st, skipped + sk, exact_handoffs + ex
        assert sure <= clamps <= sure + unsure, f"{name}: oracle clamped {clamps} steps, plain rule {sure} (+{unsure} undecided)"
        if case.expect in ("clamp+", "clamp-"):
            assert unsure == 0 and sure == clamps >= 1, (name, sure, unsure, clamps)
    assert skipped <= 0.10 * steps, (skipped, steps)
    assert exact_handoffs >= 40, exact_handoffs
    print(f"\nsteps: {steps} updating steps, {skipped} skipped for cond(H) > 1e5 ({100.0 * skipped / steps:.1f} %), "
          f"{exact_handoffs} level ends checked at 2 ulp alone")


def test_plain_statement_converges():
    """The plain statement is a matcher in its own right: iterated in float64 from a near hint on the 1024^2 map it
    settles where the oracle's match does (a check of the plain module, not of the oracle)."""
    geo = K.Geo(0.05, 1024, 1024, (0.5, 0.5), 1)
    case = K.Case("conv", geo, K.scan(0.05, 577), (0.25, 0.0, 0.08))
    pose, _, _, tr = K.run_oracle(case, trace=True)
    L = geo.pyramid()[0]
    l0 = K.maps(geo)[0][0]
    est = tr[0, :3].astype(np.float64)
    for _ in range(6):
        est, H, b, upd, cl = P.gn_step(L, l0, est, case.pts)
    w = P.world_from_map(L, est)
    assert np.abs(w[:2] - pose[:2]).max() < 2e-3 and abs(w[2] - pose[2]) < 2e-4, (w, pose)
