"""Write tests/golden/plicp_plain_steps.npz: single PL-ICP iterations computed by the plain 50-digit
reference (tests/ref/plicp_plain.py), for tests/test_plicp_cpu.py (the oracle against them) and
tests/test_plicp_gpu.py (the kernel against them).

Scans: the synthetic room (slam2d.synth) seen by a 270-degree lidar of 360 and of 720 beams, range noise 0,
0.01 and 0.03 m, readings rounded to float32 as a LaserScan carries them (and stored so).  Cases: per
(beams, noise) 3 consecutive scan pairs with the node's parameters; on the 360-beam, 0.01 m scans one pair
each with use_point_to_line_distance = 0, outliers_remove_doubles = 0, max_correspondence_dist = 0.3 and the
first guess (0.3, -0.2, 0.1).  Every case is a chain of 6 iterations: step s starts from x_old[s], the plain
reference's result is stored, and the oracle's result of that one iteration (max_iterations = 1) is the next
x_old -- so the stored x_old are the poses the oracle and the kernel really pass through.

The file holds numbers only: scans, parameters, x_old and the reference's x_new / nvalid / error.

Seed: SEED below is the first one tried; no step of it has a decision (a trimming tie, a cell boundary
between libm's and detmath's atan) on which the oracle and the plain reference fall on different sides.  If
an input is ever changed so that one does, change the seed and say so here -- not the test's assertion.

    python tests/ref/make_plicp_golden.py [output.npz]
"""
import math
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
for p in (HERE, os.path.join(REPO, "oracle"), os.path.join(REPO, "creating-2d-laser-slam-from-scratch_amd", "python")):
    if p not in sys.path:
        sys.path.insert(0, p)
import plicp_plain as P  # noqa: E402

GOLDEN = os.path.join(REPO, "tests", "golden", "plicp_plain_steps.npz")
SEED = 20240
STEPS = 6
BEAMS = (360, 720)
NOISES = (0.0, 0.01, 0.03)
PAIRS = 3
ANGLE_MIN = -0.75 * math.pi


def scans(n, noise, seed):
    """PAIRS + 1 consecutive scans [PAIRS + 1, n] float32 (-1 = invalid), angle_inc."""
    from slam2d import synth
    from slam2d.plicp import laser_scan_to_readings

    inc = 1.5 * math.pi / (n - 1)
    ang = ANGLE_MIN + inc * np.arange(n, dtype=np.float64)
    gt = synth.trajectory(PAIRS + 1, 0.3)
    R = synth.cast_ranges(gt, synth.world_segments(), n, ang)
    R = R + np.random.default_rng(seed).normal(0.0, noise, R.shape)
    return laser_scan_to_readings(R, 0.1, 29.9).astype(np.float32), inc


def case_list():
    """[(beams, noise index, ref scan, sens scan, parameter overrides, first guess)]"""
    cases = []
    for n in BEAMS:
        for k in range(len(NOISES)):
            for p in range(PAIRS):
                cases.append((n, k, p, p + 1, {}, (0.0, 0.0, 0.0)))
    for p, over, guess in ((0, dict(use_point_to_line_distance=0), (0.0, 0.0, 0.0)),
                           (1, dict(outliers_remove_doubles=0), (0.0, 0.0, 0.0)),
                           (2, dict(max_correspondence_dist=0.3), (0.0, 0.0, 0.0)),
                           (0, {}, (0.3, -0.2, 0.1))):
        cases.append((360, 1, p, p + 1, over, guess))
    return cases


def param_vector(over):
    d = dict(P.DEFAULTS)
    d.update(over)
    return np.array([float(d[k]) for k in P.PARAM_NAMES], np.float64)


def oracle_params(vec):
    import oracle as O

    p = O.pl_default_params()
    for k, v in zip(P.PARAM_NAMES, vec):
        setattr(p, k, type(getattr(p, k))(v))
    return p


def compute():
    """The fixture's arrays, from the plain reference (the chain's x_old from the oracle)."""
    import oracle as O

    S = {}
    for n in BEAMS:
        S[n] = np.stack([scans(n, noise, SEED + 7 * k + n)[0] for k, noise in enumerate(NOISES)])  # [noise, scan, n]
    cases = case_list()
    C = len(cases)
    out = dict(param_names=np.array(P.PARAM_NAMES), angle_min=np.float64(ANGLE_MIN),
               case_beams=np.zeros(C, np.int32), case_noise=np.zeros(C, np.int32), case_ref=np.zeros(C, np.int32),
               case_sens=np.zeros(C, np.int32), case_params=np.zeros((C, len(P.PARAM_NAMES))),
               x_old=np.zeros((C, STEPS, 3)), x_new=np.zeros((C, STEPS, 3)), nvalid=np.zeros((C, STEPS), np.int32),
               error=np.zeros((C, STEPS)))
    for n in BEAMS:
        out[f"scans{n}"] = S[n]
    for c, (n, k, a, b, over, guess) in enumerate(cases):
        inc = 1.5 * math.pi / (n - 1)
        theta = ANGLE_MIN + inc * np.arange(n, dtype=np.float64)
        ref, sens = S[n][k, a].astype(np.float64), S[n][k, b].astype(np.float64)
        vec = param_vector(over)
        one = oracle_params(vec)
        one.max_iterations = 1
        out["case_beams"][c], out["case_noise"][c], out["case_ref"][c], out["case_sens"][c] = n, k, a, b
        out["case_params"][c] = vec
        x = np.array(guess, np.float64)
        for s in range(STEPS):
            r = P.step(ref, sens, theta, x, dict(zip(P.PARAM_NAMES, vec)))
            assert r["status"] == "ok", (c, s, r["status"])
            out["x_old"][c, s], out["x_new"][c, s] = x, r["x_new"]
            out["nvalid"][c, s], out["error"][c, s] = r["nvalid"], r["error"]
            o = O.plicp(ref, sens, ANGLE_MIN, inc, x, one, reduce_threads=256)
            assert o["valid"], (c, s)
            x = o["x"].copy()
    return out


def main(path):
    import oracle as O

    out = compute()
    np.savez_compressed(path, **out)
    # report the oracle-vs-plain deviation of what was written (the test's bars are 4 x these maxima)
    dx = de = 0.0
    flips = 0
    for c in range(out["x_old"].shape[0]):
        n = int(out["case_beams"][c])
        inc = 1.5 * math.pi / (n - 1)
        sc = out[f"scans{n}"][out["case_noise"][c]].astype(np.float64)
        one = oracle_params(out["case_params"][c])
        one.max_iterations = 1
        for s in range(STEPS):
            for T in (0, 256):
                o = O.plicp(sc[out["case_ref"][c]], sc[out["case_sens"][c]], ANGLE_MIN, inc, out["x_old"][c, s], one,
                            reduce_threads=T)
                flips += o["nvalid"] != out["nvalid"][c, s]
                dx = max(dx, float(np.abs(o["x"] - out["x_new"][c, s]).max()))
                de = max(de, abs(o["error"] - out["error"][c, s]))
    print(f"{out['x_old'].shape[0]} cases x {STEPS} steps: nvalid differs in {flips} oracle runs, "
          f"max |x - plain| {dx:.3e}, max |error - plain| {de:.3e}")
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else GOLDEN)
