"""GPU parity of the PL-ICP path (lesson3 front-end): pl_icp_kernel through the C-ABI vs the CPU
restatement oracle/plicp_oracle.c in the kernel's summation order.  Bit-exact in every output
(x, valid, iterations, nvalid, error).  CSM itself is absent: parity against CSM is unpinned; single
iterations are held to the plain 50-digit reference (tests/ref/plicp_plain.py) through its stored results."""
import ctypes as C
import functools
import math
import os

import numpy as np
import pytest

import oracle as O
from slam2d import synth
from slam2d._lib import Slam2dError
from slam2d.plicp import PLICP, PlResult, default_params, laser_scan_to_readings

pytestmark = pytest.mark.gpu


def _pairs(num, seed, noise=0.01, step=1, phase=0.3):
    rng = np.random.default_rng(seed)
    ang = synth.beam_angles().astype(np.float64)
    gt = synth.trajectory(num * step + 1, phase)
    R = synth.cast_ranges(gt, synth.world_segments())
    R = R + rng.normal(0, noise, R.shape)
    R = laser_scan_to_readings(R, 0.1, 29.9)
    pairs = [(R[k * step], R[k * step + 1]) for k in range(num)]
    return pairs, float(ang[0]), float(ang[1] - ang[0])


def _same(g, o):
    np.testing.assert_array_equal(g["x"], o["x"])
    assert g["valid"] == o["valid"] and g["iterations"] == o["iterations"] and g["nvalid"] == o["nvalid"]
    assert g["error"] == o["error"]


@pytest.mark.parametrize("noise", [0.0, 0.01, 0.03])
def test_consecutive_scans_bitexact(gpu, noise):
    pairs, amin, inc = _pairs(6, 3, noise)
    pl = PLICP(1, 1081)
    for ref, sens in pairs:
        _same(pl.icp(ref, sens, amin, inc), O.plicp(ref, sens, amin, inc, reduce_threads=256))


def test_first_guess_and_wide_motion(gpu):
    """Keyframe-style pairs (several scans apart) with a non-zero first guess (GetPrediction)."""
    pairs, amin, inc = _pairs(4, 9, 0.01, step=5)
    pl = PLICP(1, 1081)
    for k, (ref, sens) in enumerate(pairs):
        g = (0.3 * k - 0.2, 0.05, 0.02 * k)
        _same(pl.icp(ref, sens, amin, inc, g), O.plicp(ref, sens, amin, inc, g, reduce_threads=256))


def test_sparse_and_failing_scans(gpu):
    """Mostly invalid rays (fewer than 5 % correspondences -> valid = 0) and a short scan."""
    pairs, amin, inc = _pairs(2, 5)
    ref, sens = pairs[0]
    sparse = sens.copy()
    sparse[::1] = -1.0
    sparse[::40] = sens[::40]
    pl = PLICP(1, 1081)
    _same(pl.icp(ref, sparse, amin, inc), O.plicp(ref, sparse, amin, inc, reduce_threads=256))
    r_short, s_short = ref[300:700].copy(), sens[300:700].copy()
    _same(pl.icp(r_short, s_short, amin + 300 * inc, inc), O.plicp(r_short, s_short, amin + 300 * inc, inc, reduce_threads=256))


def test_batch_device(gpu):
    import torch

    pairs, amin, inc = _pairs(12, 21, 0.01)
    B = len(pairs)
    ref = torch.from_numpy(np.stack([p[0] for p in pairs])).cuda()
    sens = torch.from_numpy(np.stack([p[1] for p in pairs])).cuda()
    guess = torch.zeros((B, 3), dtype=torch.float64, device="cuda")
    out = torch.zeros((B, C.sizeof(PlResult)), dtype=torch.uint8, device="cuda")
    pl = PLICP(B, 1081)
    pl.icp_batch_device(B, 1081, amin, inc, ref.data_ptr(), sens.data_ptr(), guess.data_ptr(), out.data_ptr(),
                        torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    raw = out.cpu().numpy()
    for b in range(B):
        r = PlResult.from_buffer_copy(raw[b].tobytes())
        g = dict(x=np.array(r.x[:]), valid=bool(r.valid), iterations=r.iterations, nvalid=r.nvalid, error=r.error)
        _same(g, O.plicp(pairs[b][0], pairs[b][1], amin, inc, reduce_threads=256))


@pytest.mark.parametrize("n_beams,scale", [(1440, 1.0), (1081, 0.2), (1440, 0.12)])
def test_full_circle_and_near_scans(gpu, n_beams, scale):
    """The correspondence search prunes the polar interval by the angular distance bound (kept
    candidates visited in the same order): a 360-degree scan (1440 beams from -135 deg, wrapping past
    pi) and scaled-down worlds whose points sit around the pruning threshold (2.02 m) -- bit-exact vs
    the oracle's exhaustive interval scan."""
    rng = np.random.default_rng(77 + n_beams)
    ang0 = float(synth.ANGLE_MIN)
    inc = float(np.float64(synth.ANGLE_INC))
    gt = synth.trajectory(5, 1.1)
    R = synth.cast_ranges(gt, synth.world_segments(), n_beams) * scale
    R = R + rng.normal(0, 0.01 * scale, R.shape)
    R = laser_scan_to_readings(R, 0.05, 29.9)
    pl = PLICP(1, n_beams)
    for k in range(4):
        _same(pl.icp(R[k], R[k + 1], ang0, inc), O.plicp(R[k], R[k + 1], ang0, inc, reduce_threads=256))


# ------------------------------------------------------------------------------------------------------------
# The whole kernel: every instantiation (pl_launch picks pl_icp_kernel<2|4|5|6|8> from ceil(n / 256)), every
# pl_params field at a non-default value, every way out of the loop, degenerate data, the batch call and
# pl_icp_ldp -- all bit-equal to the oracle in the kernel's summation order; then single iterations against
# the plain 50-digit reference (tests/golden/plicp_plain_steps.npz).  The oracle's results are computed once
# per input (lru_cache) and shared by the tests that need them.
AMIN = -0.75 * math.pi


@functools.lru_cache(maxsize=None)
def _scans(n, num, seed, noise=0.01, phase=0.3, amin=AMIN):
    """num consecutive scans of n beams over 270 degrees (angle_inc = 1.5 pi / (n - 1)); readings, amin, inc."""
    inc = 1.5 * math.pi / (n - 1)
    ang = amin + inc * np.arange(n, dtype=np.float64)
    R = synth.cast_ranges(synth.trajectory(num, phase), synth.world_segments(), n, ang)
    R = R + np.random.default_rng(seed).normal(0, noise, R.shape)
    R = laser_scan_to_readings(R, 0.1, 29.9)
    R.setflags(write=False)
    return R, amin, inc


def _gp(over=()):
    """pl_params of the product and plo_params of the oracle with the same overrides."""
    g, o = default_params(), O.pl_default_params()
    for k, v in dict(over).items():
        assert hasattr(g, k)
        setattr(g, k, v)
        setattr(o, k, v)
    return g, o


def _oracle(ref, sens, amin, inc, guess=(0.0, 0.0, 0.0), over=()):
    return O.plicp(ref, sens, amin, inc, guess, _gp(over)[1], reduce_threads=256)


# ---- a. ray-count sweep: <2> n <= 512, <4> <= 1024, <5> <= 1280, <6> <= 1536, <8> <= 2048; n < 256 leaves
# threads without a ray, n < 64 whole waves
SWEEP = (2, 3, 16, 63, 64, 65, 255, 256, 257, 512, 513, 1024, 1025, 1280, 1281, 1536, 1537, 2047, 2048)


@functools.lru_cache(maxsize=None)
def _sweep_oracle(n):
    R, amin, inc = _scans(n, 3, 100 + n)
    res = tuple(_oracle(R[k], R[k + 1], amin, inc) for k in range(2))
    for r in res:   # the sweep must not turn into an all-failing one unnoticed
        if n <= 3:
            assert not r["valid"]
        else:
            assert r["valid"] and 2 <= r["iterations"] <= 10, (n, r)
    return res


def _sweep_check(pl, n):
    R, amin, inc = _scans(n, 3, 100 + n)
    for k, o in enumerate(_sweep_oracle(n)):
        _same(pl.icp(R[k], R[k + 1], amin, inc), o)


@pytest.mark.parametrize("n", SWEEP)
def test_ray_count_sweep_own_context(gpu, n):
    _sweep_check(PLICP(1, n), n)


def test_ray_count_sweep_one_context(gpu):
    """One context of 2048 rays serves every n, ascending then descending: five instantiations, one context."""
    pl = PLICP(1, 2048)
    for n in SWEEP + SWEEP[::-1]:
        _sweep_check(pl, n)


# ---- b. parameters at n = 720 (<4>)
PARAM_SETS = (
    dict(use_point_to_line_distance=0),
    dict(outliers_remove_doubles=0),
    dict(max_iterations=1),
    dict(max_iterations=64),
    dict(epsilon_xy=1e-2, epsilon_theta=1e-2),
    dict(max_correspondence_dist=0.05),
    dict(max_correspondence_dist=5.0),
    dict(outliers_maxPerc=1.0),
    dict(outliers_adaptive_order=0.0),
    dict(outliers_adaptive_mult=0.5),
    dict(max_angular_correction_deg=1.0),
    dict(max_linear_correction=0.01),
    dict(max_angular_correction_deg=180.0, max_linear_correction=10.0),
    # far past the 10 iterations of a default run (s_hash has 64 slots): 18 .. 64 on these pairs
    dict(max_iterations=64, use_point_to_line_distance=0),
    # the two interval limits change nothing on these pairs one at a time (atan(1 / |w|) or 45 degrees keeps the
    # interval wide); together they leave a few cells, so a kernel that ignored either would show here
    dict(max_angular_correction_deg=1.0, max_linear_correction=0.01),
)
# every set runs on 3 pairs from a zero first guess and on the same pairs from one that needs more iterations
PARAM_GUESSES = ((0.0, 0.0, 0.0), (0.6, 0.4, -0.3))


@functools.lru_cache(maxsize=None)
def _param_oracle(idx):
    R, amin, inc = _scans(720, 4, 720)
    over = tuple(sorted(PARAM_SETS[idx].items())) if idx >= 0 else ()
    return tuple(_oracle(R[k], R[k + 1], amin, inc, g, over) for g in PARAM_GUESSES for k in range(3))


def test_param_sets_do_what_they_are_for():
    """From the oracle alone: the sets reach the behaviour they were chosen for, and every field shows."""
    base = _param_oracle(-1)
    it = lambda idx: [r["iterations"] for r in _param_oracle(idx)]
    assert it(2) == [1] * 6
    assert all(2 <= i <= 3 for i in it(4)[:3])
    assert not any(r["valid"] for r in _param_oracle(8))
    assert max(it(3)) > 10 and max(it(13)) == 64
    key = lambda r: (tuple(r["x"]), r["valid"], r["iterations"], r["nvalid"], r["error"])
    for idx in range(len(PARAM_SETS)):
        differs = any(key(a) != key(b) for a, b in zip(_param_oracle(idx), base))
        assert differs == (idx not in (10, 11, 12)), idx


@pytest.mark.parametrize("idx", range(len(PARAM_SETS)))
def test_params_at_create_and_by_set_params(gpu, idx):
    R, amin, inc = _scans(720, 4, 720)
    want = _param_oracle(idx)
    made = PLICP(1, 720, _gp(PARAM_SETS[idx])[0])
    later = PLICP(1, 720)
    later.set_params(_gp(PARAM_SETS[idx])[0])
    for q, g in enumerate(PARAM_GUESSES):
        for k in range(3):
            _same(made.icp(R[k], R[k + 1], amin, inc, g), want[3 * q + k])
            _same(later.icp(R[k], R[k + 1], amin, inc, g), want[3 * q + k])
    later.set_params(default_params())
    _same(later.icp(R[0], R[1], amin, inc), _param_oracle(-1)[0])


@pytest.mark.parametrize("bad", [0, 65, -1])
def test_max_iterations_out_of_range_is_refused(gpu, bad):
    p = default_params()
    p.max_iterations = bad
    with pytest.raises(Slam2dError):
        PLICP(1, 720, p)
    R, amin, inc = _scans(720, 4, 720)
    pl = PLICP(1, 720)
    with pytest.raises(Slam2dError):
        pl.set_params(p)
    _same(pl.icp(R[0], R[1], amin, inc), _param_oracle(-1)[0])   # the refused set changed nothing


# ---- c. exits
@functools.lru_cache(maxsize=None)
def _exit_cases():
    """[(ref, sens, amin, inc, guess, overrides, oracle result)]"""
    R, amin, inc = _scans(720, 4, 720)
    R0 = _scans(720, 4, 721, 0.0)[0]
    Q = _scans(720, 4, 721)[0]
    S3, a3, i3 = _scans(3, 3, 103)
    eps = (("epsilon_theta", 1e-2), ("epsilon_xy", 1e-2))
    sparse = np.where(np.arange(720) % 40 == 0, R[1], -1.0)
    cases = [(R0[k], R0[k + 1], amin, inc, (0.0, 0.0, 0.0), ()) for k in range(3)]
    cases += [(R[k], R[k + 1], amin, inc, (0.0, 0.0, 0.0), ()) for k in range(3)]
    cases += [(Q[k], Q[k + 1], amin, inc, (0.0, 0.0, 0.0), ()) for k in range(3)]
    cases += [(R[k], R[k + 1], amin, inc, (0.0, 0.0, 0.0), eps) for k in range(3)]
    cases += [(R[0], R[0], amin, inc, (0.0, 0.0, 0.0), ())]                       # identical scans: 1 iteration
    cases += [(R[0], R[1], amin, inc, (0.0, 0.0, 0.0), (("max_iterations", 1),))]
    cases += [(R[0], R[1], amin, inc, (0.0, 0.0, 0.0), (("max_correspondence_dist", 0.05),))]
    cases += [(R[k], R[k + 1], amin, inc, (0.0, 0.0, g), ()) for k in range(3) for g in (-3.1, 3.1)]
    cases += [(R[0], sparse, amin, inc, (0.0, 0.0, 0.0), ())]
    # a failed solve through the C-ABI: 3 rays leave at most one correspondence (ray 1), so A = n n^T is singular
    cases += [(S3[0], S3[1], a3, i3, (0.0, 0.0, 0.0), ())]
    # ... and a trimming that keeps only the smallest error (adaptive_order = 0), rank one again
    cases += [(R[0], R[1], amin, inc, (0.0, 0.0, 0.0), (("outliers_adaptive_order", 0.0),))]
    return tuple(c + (_oracle(*c[:5], over=c[5]),) for c in cases)


def test_every_exit_is_taken_and_bit_equal(gpu):
    """converged (epsilon), loop (a repeated correspondence hash), max_it, few_corr (< 5 % correspondences) and
    solve: the last one is reached through the C-ABI by inputs that leave one correspondence (detA = 0 exactly);
    |h| = 0 and a non-finite estimate were not reached by any input tried."""
    cases = _exit_cases()
    exits = {c[6]["exit"] for c in cases}
    assert exits >= {"converged", "loop", "max_it", "few_corr", "solve"}, exits
    for ref, sens, amin, inc, guess, over, o in cases:
        _same(PLICP(1, ref.shape[0], _gp(over)[0]).icp(ref, sens, amin, inc, guess), o)


# ---- d. degenerate data at n = 720, angle_min = -360 inc: theta[360] == 0.0 exactly
def _degenerate():
    n = 720
    inc = 1.5 * math.pi / (n - 1)
    amin = -360 * inc
    ang = amin + inc * np.arange(n, dtype=np.float64)
    assert ang[360] == 0.0
    D = synth.cast_ranges(synth.trajectory(3, 0.3), synth.world_segments(), n, ang)
    D = laser_scan_to_readings(D + np.random.default_rng(5).normal(0, 0.01, D.shape), 0.1, 29.9)
    ref, sens = D[0], D[1]
    assert sens[360] > 0.0
    quant = lambda a: np.where(a > 0, np.round(a * 8) / 8, -1.0)
    with np.errstate(divide="ignore"):
        wall = lambda d: np.where(np.abs(ang) < 1.0, d / np.cos(ang), -1.0)
    nan_s, nan_r = sens.copy(), ref.copy()
    nan_s[::7] = np.nan
    nan_r[5::11] = np.nan
    none = np.full(n, -1.0)
    z = (0.0, 0.0, 0.0)
    S40, a40, i40 = _scans(40, 2, 40)
    return {
        "same": (ref, ref, amin, inc, z),
        "eighths": (quant(ref), quant(sens), amin, inc, z),          # duplicate trimming keys
        "wall": (wall(3.0), wall(2.9), amin, inc, z),                # collinear: an ill-conditioned solve
        "wall_itself": (wall(3.0), wall(3.0), amin, inc, z),
        "nan": (nan_r, nan_s, amin, inc, z),
        "no_ref": (none, sens, amin, inc, z),
        "no_sens": (ref, none, amin, inc, z),
        "no_rays": (none, none, amin, inc, z),
        "ref_every_50th": (np.where(np.arange(n) % 50 == 0, ref, -1.0), sens, amin, inc, z),
        "point_at_origin": (ref, sens, amin, inc, (-sens[360], 0.0, 0.0)),   # ray 360 lands on (0, 0) exactly
        "turned_2.5": (ref, sens, amin, inc, (0.0, 0.0, 2.5)),
        "moved_3": (ref, sens, amin, inc, (3.0, 0.0, 0.0)),
        "guess_far": (ref, sens, amin, inc, (0.5, -0.5, 0.7)),
        "40_beams": (S40[0], S40[1], a40, i40, z),
    }


DEGENERATE = ("same", "eighths", "wall", "wall_itself", "nan", "no_ref", "no_sens", "no_rays", "ref_every_50th",
              "point_at_origin", "turned_2.5", "moved_3", "guess_far", "40_beams")


@pytest.mark.parametrize("name", DEGENERATE)
def test_degenerate_data(gpu, name):
    cases = _degenerate()
    assert set(cases) == set(DEGENERATE)
    ref, sens, amin, inc, guess = cases[name]
    o = _oracle(ref, sens, amin, inc, guess)
    if name.startswith("no_"):
        assert not o["valid"] and o["exit"] == "few_corr"
    if name in ("same", "wall_itself"):
        assert o["valid"] and o["iterations"] == 1
    _same(PLICP(1, ref.shape[0]).icp(ref, sens, amin, inc, guess), o)


# ---- e. batch
def _batch(pl, count, n, amin, inc, ref, sens, guess, guard=64, fill=0xA5):
    """pl_icp_batch_device into a buffer pre-filled with `fill`, `guard` bytes after the last pl_result."""
    import torch

    size = C.sizeof(PlResult)
    out = torch.full((count * size + guard,), fill, dtype=torch.uint8, device="cuda")
    d_ref, d_sens = torch.from_numpy(np.array(ref, np.float64)).cuda(), torch.from_numpy(np.array(sens, np.float64)).cuda()
    d_guess = None if guess is None else torch.from_numpy(np.array(guess, np.float64)).cuda()
    pl.icp_batch_device(count, n, amin, inc, d_ref.data_ptr(), d_sens.data_ptr(), 0 if d_guess is None else d_guess.data_ptr(),
                        out.data_ptr(), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    raw = out.cpu().numpy()
    assert np.all(raw[count * size:] == fill), "bytes after the last pl_result were written"
    res = []
    for b in range(count):
        r = PlResult.from_buffer_copy(raw[b * size:(b + 1) * size].tobytes())
        res.append(dict(x=np.array(r.x[:]), valid=bool(r.valid), iterations=r.iterations, nvalid=r.nvalid, error=r.error))
    return res, raw


@pytest.mark.parametrize("n,count", [(64, 48), (2048, 12)])
def test_batch_guesses_failures_and_guard(gpu, n, count):
    R, amin, inc = _scans(n, count + 1, 5000 + n)
    ref, sens = R[:count].copy(), R[1:count + 1].copy()
    rng = np.random.default_rng(n)
    guess = rng.normal(0.0, 1.0, (count, 3)) * np.array([0.05, 0.05, 0.02])
    sens[3] = -1.0                       # failing pairs between good ones
    guess[5] = (0.0, 0.0, -3.1)
    guess[count - 2] = (40.0, 0.0, 0.0)
    want = [_oracle(ref[b], sens[b], amin, inc, tuple(guess[b])) for b in range(count)]
    assert not want[3]["valid"] and not want[count - 2]["valid"]
    assert all(want[b]["valid"] for b in (2, 4, 6, count - 3, count - 1))
    pl = PLICP(count, n)
    got, _ = _batch(pl, count, n, amin, inc, ref, sens, guess)
    for b in range(count):
        _same(got[b], want[b])
    # neighbours of the failing pairs: the same results as when run alone
    one = PLICP(1, n)
    for b in (2, 4, 6, count - 3, count - 1):
        _same(one.icp(ref[b], sens[b], amin, inc, guess[b]), got[b])
    # d_first_guess = NULL is the zero guess
    null, _ = _batch(pl, count, n, amin, inc, ref, sens, None)
    zero, _ = _batch(pl, count, n, amin, inc, ref, sens, np.zeros((count, 3)))
    for b in range(count):
        _same(null[b], zero[b])
        _same(null[b], _oracle(ref[b], sens[b], amin, inc))
    # count = 0: PL_OK, nothing written
    _, raw = _batch(pl, 0, n, amin, inc, ref, sens, guess, guard=256)
    assert np.all(raw == 0xA5)


def test_batch_refuses_bad_arguments(gpu):
    R, amin, inc = _scans(64, 5, 5064)
    pl = PLICP(4, 64)
    ref, sens, guess = R[:4], R[1:5], np.zeros((4, 3))
    for count, n, a_inc in ((5, 64, inc), (-1, 64, inc), (4, 65, inc), (4, 1, inc), (4, 0, inc), (4, 64, 0.0), (4, 64, -inc),
                            (4, 64, float("nan"))):
        with pytest.raises(Slam2dError):
            _batch(pl, count, n, amin, a_inc, ref, sens, guess)
    got, _ = _batch(pl, 4, 64, amin, inc, ref, sens, guess)       # the context still works
    for b in range(4):
        _same(got[b], _oracle(ref[b], sens[b], amin, inc))


# ---- f. pl_icp_ldp
@pytest.mark.parametrize("n", [720, 1081])
def test_icp_ldp(gpu, n):
    """theta[] as LaserScanToLDP builds it from the LaserScan's float32 angle_min / angle_increment, valid[]
    arrays that disagree with the readings' signs, non-default parameters."""
    R, amin, inc = _scans(n, 3, 900 + n)
    theta = float(np.float32(amin)) + np.arange(n, dtype=np.float64) * float(np.float32(inc))
    over = (("max_correspondence_dist", 0.5), ("max_iterations", 20), ("outliers_maxPerc", 0.95))
    pl = PLICP(1, n, _gp(over)[0])
    for k in range(2):
        ref, sens = R[k].copy(), R[k + 1].copy()
        rv, sv = (ref > 0).astype(np.int32), (sens > 0).astype(np.int32)
        rv[10:40] = 0            # valid readings marked invalid
        sv[::9] = 0
        ref[100:110] = -1.0      # invalid readings marked valid: they stay invalid
        rv[100:110] = 1
        sens[200:205] = 0.0
        sv[200:205] = 1
        o_ref, o_sens = np.where((rv != 0) & (ref > 0), ref, -1.0), np.where((sv != 0) & (sens > 0), sens, -1.0)
        guess = (0.02, -0.01, 0.01 * k)
        want = O.plicp_theta(theta, o_ref, o_sens, guess, _gp(over)[1], reduce_threads=256)
        assert want["valid"]
        _same(pl.icp_ldp(theta, ref, sens, rv, sv, guess), want)
        # valid = NULL: the readings' signs decide
        _same(pl.icp_ldp(theta, o_ref, o_sens, None, None, guess), want)
    bent = theta.copy()
    bent[n // 2] += 0.01 * inc
    for bad in (theta[::-1].copy(), bent, np.full(n, theta[0])):
        with pytest.raises(Slam2dError):
            pl.icp_ldp(bad, R[0], R[1])


# ---- g. single iterations against the plain 50-digit reference (tests/test_plicp_cpu.py has the bars' origin)
X_BAR, ERR_BAR = 4 * 1.4199e-14, 4 * 1.5632e-13


def test_single_iterations_against_plain_reference(gpu):
    z = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "plicp_plain_steps.npz"))
    names = [str(s) for s in z["param_names"]]
    amin = float(z["angle_min"])
    pl = PLICP(1, 720)
    steps = 0
    dx = de = 0.0
    for c in range(z["x_old"].shape[0]):
        n = int(z["case_beams"][c])
        inc = 1.5 * math.pi / (n - 1)
        sc = z[f"scans{n}"][z["case_noise"][c]].astype(np.float64)
        over = dict(zip(names, z["case_params"][c]))
        over.update(max_iterations=1)
        p = default_params()
        for k, v in over.items():
            setattr(p, k, type(getattr(p, k))(v))
        pl.set_params(p)
        for s in range(z["x_old"].shape[1]):
            g = pl.icp(sc[z["case_ref"][c]], sc[z["case_sens"][c]], amin, inc, z["x_old"][c, s])
            assert g["valid"] and g["iterations"] == 1
            assert g["nvalid"] == z["nvalid"][c, s], (c, s)
            dx = max(dx, float(np.abs(g["x"] - z["x_new"][c, s]).max()))
            de = max(de, abs(g["error"] - z["error"][c, s]))
            steps += 1
    print(f"{steps} steps: max |x - plain| {dx:.4e}, max |error - plain| {de:.4e}")
    assert steps == 132
    assert dx <= X_BAR and de <= ERR_BAR, (dx, de)
