"""The PL-ICP oracle (oracle/plicp_oracle.c) against the plain 50-digit reference of one ICP iteration
(tests/ref/plicp_plain.py, stored in tests/golden/plicp_plain_steps.npz by tests/ref/make_plicp_golden.py):
22 cases x 6 chained steps (360 and 720 beams, noise 0 / 0.01 / 0.03 m, the node's parameters; plus
use_point_to_line_distance = 0, outliers_remove_doubles = 0, max_correspondence_dist = 0.3 and a first guess
of (0.3, -0.2, 0.1)), each run through the oracle with max_iterations = 1 in both summation orders
(reduce_threads 0 and 256).

Measured on these 132 steps x 2 orders (oracle vs plain): nvalid equal in every run;
    max |x_new - plain|  = 1.4199e-14   -> bar 4 x = 5.6796e-14  (reduce_threads 0; 1.9013e-15 with 256)
    max |error - plain|  = 1.5632e-13   -> bar 4 x = 6.2528e-13  (errors of 3 .. 14)
tests/test_plicp_gpu.py holds the kernel to the same stored values and bars.
"""
import math
import os
import sys

import numpy as np
import pytest

import oracle as O

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden", "plicp_plain_steps.npz")

X_MEASURED, ERR_MEASURED = 1.4199e-14, 1.5632e-13
X_BAR, ERR_BAR = 4 * X_MEASURED, 4 * ERR_MEASURED


def golden_cases(path=GOLDEN):
    """[(ref, sens, angle_min, angle_inc, params dict, x_old [S, 3], x_new [S, 3], nvalid [S], error [S])]"""
    z = np.load(path)
    names = [str(s) for s in z["param_names"]]
    amin = float(z["angle_min"])
    out = []
    for c in range(z["x_old"].shape[0]):
        n = int(z["case_beams"][c])
        sc = z[f"scans{n}"][z["case_noise"][c]].astype(np.float64)
        out.append((sc[z["case_ref"][c]], sc[z["case_sens"][c]], amin, 1.5 * math.pi / (n - 1),
                    dict(zip(names, z["case_params"][c])), z["x_old"][c], z["x_new"][c], z["nvalid"][c], z["error"][c]))
    return out


def one_iteration_params(d):
    p = O.pl_default_params()
    for k, v in d.items():
        setattr(p, k, type(getattr(p, k))(v))
    p.max_iterations = 1
    return p


@pytest.mark.parametrize("reduce_threads", [0, 256])
def test_oracle_matches_plain_reference_every_step(reduce_threads):
    cases = golden_cases()
    assert len(cases) == 22
    steps = 0
    dx = de = 0.0
    for ref, sens, amin, inc, pd, x_old, x_new, nvalid, error in cases:
        p = one_iteration_params(pd)
        for s in range(x_old.shape[0]):
            o = O.plicp(ref, sens, amin, inc, x_old[s], p, reduce_threads=reduce_threads)
            assert o["valid"] and o["iterations"] == 1 and o["exit"] in ("max_it", "converged")
            assert o["nvalid"] == nvalid[s], (steps, o["nvalid"], nvalid[s])
            dx = max(dx, float(np.abs(o["x"] - x_new[s]).max()))
            de = max(de, abs(o["error"] - error[s]))
            steps += 1
    print(f"reduce_threads {reduce_threads}: {steps} steps, max |x - plain| {dx:.4e}, max |error - plain| {de:.4e}")
    assert steps == 132
    assert dx <= X_BAR and de <= ERR_BAR, (dx, de)


def test_chain_is_the_oracles_own():
    """x_old of step s + 1 is the oracle's result of step s (reduce_threads = 256): the stored poses are the
    ones the oracle and the kernel pass through, bit for bit."""
    for ref, sens, amin, inc, pd, x_old, *_ in golden_cases():
        p = one_iteration_params(pd)
        for s in range(x_old.shape[0] - 1):
            o = O.plicp(ref, sens, amin, inc, x_old[s], p, reduce_threads=256)
            np.testing.assert_array_equal(o["x"], x_old[s + 1])


def test_fixture_is_what_the_plain_reference_gives_now():
    pytest.importorskip("mpmath")
    sys.path.insert(0, os.path.join(HERE, "ref"))
    try:
        import make_plicp_golden as M
    finally:
        sys.path.pop(0)
    now = M.compute()
    z = np.load(GOLDEN)
    assert sorted(now) == sorted(z.files)
    for k in z.files:
        np.testing.assert_array_equal(np.asarray(now[k]), z[k], err_msg=k)


def test_exit_field():
    """The oracle's `exit` on inputs whose way out is known by construction."""
    ref, sens, amin, inc, *_ = golden_cases()[3]
    assert O.plicp(ref, ref, amin, inc)["exit"] == "converged"            # identical scans: 1 iteration
    sparse = np.where(np.arange(sens.shape[0]) % 40 == 0, sens, -1.0)     # 2.5 % of the rays valid
    r = O.plicp(ref, sparse, amin, inc)
    assert r["exit"] == "few_corr" and not r["valid"] and r["iterations"] == 1 and len(r["hashes"]) == 0
    p = O.pl_default_params()
    p.max_iterations = 1
    r = O.plicp(ref, sens, amin, inc, params=p)
    assert r["exit"] == "max_it" and r["iterations"] == 1 and len(r["hashes"]) == 1
    r = O.plicp(ref, sens, amin, inc)
    assert r["exit"] in ("loop", "converged", "max_it") and len(r["hashes"]) == r["iterations"]
    assert (r["exit"] == "loop") == (r["hashes"][-1] in r["hashes"][:-1])
