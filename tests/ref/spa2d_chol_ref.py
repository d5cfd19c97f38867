"""ctypes loader of tests/ref/spa2d_chol_ref.c: the CPU restatement of SysSPA2d::doSPA with the direct envelope
Cholesky solve of include/slam2d/spa.h, its solve alone (chol_solve), the envelope rule, and the cases the direct
mode's tests share.  The case builders are tests/ref/spa2d_ref.py's.  Test infrastructure: nothing here is imported
by the package.

Built on demand with `gcc -O2 -ffp-contract=off` into a temporary directory, like its sibling.  SuiteSparse is absent:
cs_cholsol's own order, its AMD permutation and CHOLMOD are unpinned.
"""
from __future__ import annotations

import atexit
import ctypes as C
import math
import os
import shutil
import subprocess
import tempfile

import numpy as np

import spa2d_ref as R

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(R.REPO, "tests", "golden", "spa_chol_cases.npz")

OK, NO_FIXED, DISCONNECTED, NOT_POSDEF, FACTOR_RANGE = 0, 1, 2, 3, 4
SOLVER_PCG, SOLVER_CHOLESKY = 0, 1

_LIB = None


def lib() -> C.CDLL:
    global _LIB
    if _LIB is None:
        td = tempfile.mkdtemp(prefix="spa2d_chol_ref_")
        atexit.register(shutil.rmtree, td, ignore_errors=True)
        so = os.path.join(td, "libspa2d_chol_ref.so")
        subprocess.run(["gcc", "-O2", "-ffp-contract=off", "-std=c99", "-D_GNU_SOURCE", "-Wall", "-Werror", "-shared",
                        "-fPIC", "-I", R.CSRC, os.path.join(HERE, "spa2d_chol_ref.c"), "-o", so, "-lm"], check=True)
        L = C.CDLL(so)
        p, i, d, ll = C.c_void_p, C.c_int, C.c_double, C.c_longlong
        L.spa2d_chol_ref_compute.restype = i
        L.spa2d_chol_ref_compute.argtypes = [i, p, i, p, p, p, i, i, d, ll, C.POINTER(R.RefStats)]
        L.spa2d_chol_solve.restype = i
        L.spa2d_chol_solve.argtypes = [i, p, p, p, p]
        L.spa2d_chol_env_len.restype = ll
        L.spa2d_chol_env_len.argtypes = [i, p]
        L.spa2d_chol_first.restype = None
        L.spa2d_chol_first.argtypes = [i, i, p, i, p]
        _LIB = L
    return _LIB


_hp = R._hp


def compute(poses, ends, means, precs, prm: dict | None = None, max_factor_blocks: int = -1):
    """doSPA with the direct solve: (poses_out [n, 3], stats dict).  max_cg_iters and init_tol of prm are unused."""
    prm = R.params(**(prm or {}))
    po = np.array(poses, np.float64).reshape(-1, 3).copy()
    en = np.ascontiguousarray(ends, np.int32).reshape(-1, 2)
    me = np.ascontiguousarray(means, np.float64).reshape(-1, 3)
    pr = np.ascontiguousarray(precs, np.float64).reshape(-1, 9)
    assert len(en) == len(me) == len(pr)
    assert len(en) == 0 or (en.min() >= 0 and en.max() < len(po))
    st = R.RefStats()
    ret = lib().spa2d_chol_ref_compute(len(po), _hp(po), len(en), _hp(en), _hp(me), _hp(pr), int(prm["n_fixed"]),
                                       int(prm["niter"]), float(prm["lambda"]), int(max_factor_blocks), C.byref(st))
    stats = {k: getattr(st, k) for k in R.STAT_INTS + R.STAT_DOUBLES}
    assert ret == stats["good_iter"] and stats["cg_iters"] == 0
    return po, stats


def compute_case(case: dict, max_factor_blocks: int = -1, **over):
    prm = dict(case["params"])
    prm.update(over)
    return compute(case["poses"], case["ends"], case["means"], case["precs"], prm, max_factor_blocks)


def first_of(n: int, ends, n_fixed: int) -> np.ndarray:
    """first[] over the free nodes, as free indices (node k is entry k - n_fixed)."""
    en = np.ascontiguousarray(ends, np.int32).reshape(-1, 2)
    nf = min(n_fixed, n)
    first = np.zeros(max(n - nf, 0), np.int32)
    lib().spa2d_chol_first(n, len(en), _hp(en), n_fixed, _hp(first))
    return first


def envelope_blocks(case: dict, n_fixed: int | None = None) -> int:
    nf = case["params"]["n_fixed"] if n_fixed is None else n_fixed
    first = first_of(len(case["poses"]), case["ends"], nf)
    return int(np.sum(np.arange(len(first)) - first + 1))


def pack_env(A: np.ndarray, first) -> np.ndarray:
    """The envelope of the symmetric A [3 nb, 3 nb] as packed scalar rows: row 3k + c holds columns 3 first[k] ... 3k + c."""
    rows = [A[3 * k + c, 3 * int(first[k]):3 * k + c + 1] for k in range(len(first)) for c in range(3)]
    return np.ascontiguousarray(np.concatenate(rows) if rows else np.zeros(0), np.float64)


def unpack_env(env: np.ndarray, first) -> np.ndarray:
    """The lower-triangular matrix a packed envelope holds (zeros outside it)."""
    n = 3 * len(first)
    M = np.zeros((n, n))
    o = 0
    for k in range(len(first)):
        for c in range(3):
            w = 3 * (k - int(first[k])) + c + 1
            M[3 * k + c, 3 * int(first[k]):3 * k + c + 1] = env[o:o + w]
            o += w
    assert o == len(env)
    return M


def chol_solve(first, A_env, b):
    """The direct solve alone: (x [3 nb], ok, L_env).  A_env is not modified."""
    first = np.ascontiguousarray(first, np.int32)
    env = np.array(A_env, np.float64).copy()
    b = np.ascontiguousarray(b, np.float64)
    assert len(b) == 3 * len(first) and len(env) == lib().spa2d_chol_env_len(len(first), _hp(first))
    x = np.full(len(b), np.nan)
    ok = lib().spa2d_chol_solve(len(first), _hp(first), _hp(env), _hp(b), _hp(x))
    return x, bool(ok), env


# ---------------------------------------------------------------------------------------------- input cases
def grown_ring(n: int, seed: int) -> dict:
    """The ring whose radius grows with the node count (0.15 m per node: 9.6 m at 64 nodes), on which the PCG mode
    uses all 40 LM iterations and stops 2e-3 away from the exact-step LM."""
    rng = np.random.default_rng(seed)
    return R.graph_from_truth(R.ring_truth(n, 0.15 * n), R.ring_links(n), rng)


def case_two_hop_chain(nfree: int, seed: int, n_fixed: int = 1) -> dict:
    """nfree free nodes behind n_fixed fixed ones: a chain with two-hop links (row widths 1, 2, 3, 3, ...)."""
    n = nfree + n_fixed
    rng = np.random.default_rng(seed)
    truth = np.stack([0.5 * np.arange(n), 0.3 * np.sin(0.2 * np.arange(n)), 0.1 * np.sin(0.1 * np.arange(n))], axis=1)
    links = [(i, i + 1) for i in range(n - 1)] + [(i, i + 2) for i in range(n - 2)]
    return R.graph_from_truth(truth, links, rng, n_fixed=n_fixed)


def case_full_row(seed=41, n=40) -> dict:
    """A ring whose closure goes from the last node to the first FREE node: the last row spans the whole width."""
    rng = np.random.default_rng(seed)
    links = [(i, i + 1) for i in range(n - 1)] + [(i, i + 2) for i in range(n - 2)] + [(n - 1, 1)]
    return R.graph_from_truth(R.ring_truth(n), links, rng)


def case_mid_closures(seed=42, n=60) -> dict:
    """Closures into the middle, in both directions: rows that reach far back between rows that do not."""
    rng = np.random.default_rng(seed)
    links = R.ring_links(n) + [(50, 20), (21, 55), (30, 8), (9, 44), (58, 31)]
    return R.graph_from_truth(R.ring_truth(n, 3.0), links, rng)


def case_fixed_only(seed=43) -> dict:
    """Two fixed nodes; free node 4 is tied to the fixed nodes only (first = itself, a row of width 1 amid others)."""
    rng = np.random.default_rng(seed)
    links = [(0, 1), (1, 2), (2, 3), (0, 4), (4, 1), (3, 5), (5, 6), (2, 6), (6, 7), (5, 7)]
    return R.graph_from_truth(R.ring_truth(8, 1.5), links, rng, n_fixed=2)


def find_rejecting(lo, hi, seeds=range(400), **kw):
    """spa2d_ref.find_rejecting re-searched for the direct mode: the first seed whose outlier graph makes this
    restatement undo between lo and hi steps."""
    for s in seeds:
        c = R.case_outliers(s, **kw)
        _, st = compute_case(c)
        if st["status"] == OK and lo <= st["rejected"] <= hi and math.isfinite(st["final_cost"]):
            return s, c, st
    raise AssertionError("no seed rejects a step")


REJECT_ONCE_SEED = 24   # find_rejecting(1, 1): asserted in tests/test_spa_chol_cpu.py
REJECT_TWICE_SEED = 12  # find_rejecting(2, 2)


def case_not_posdef(seed=44) -> dict:
    """A chain of five nodes whose last constraint has the precision -I: the last node's diagonal block is
    negative, so the factor's last block column meets a pivot that is not > 0 on the first LM iteration."""
    rng = np.random.default_rng(seed)
    c = R.graph_from_truth(R.ring_truth(5), [(i, i + 1) for i in range(4)], rng)
    precs = c["precs"].copy()
    precs[3] = (-np.eye(3)).reshape(9)
    return R._case(c["poses"], c["ends"], c["means"], precs)


def golden_cases() -> dict:
    """name -> case of tests/golden/spa_chol_cases.npz."""
    return {"tiny2": R.case_tiny(2), "tiny3": R.case_tiny(3), "ring12": R.case_ring(12, 2), "ring33": R.case_ring(33, 3),
            "full_row": case_full_row(), "mid": case_mid_closures(), "fixed_only": case_fixed_only(),
            "hub_low": R.case_hub(seed=11, n=90, hub=25), "near_pi": R.case_near_pi(),
            "reject1": R.case_outliers(REJECT_ONCE_SEED), "reject2": R.case_outliers(REJECT_TWICE_SEED),
            "niter3": R.case_ring(33, 6, niter=3), "not_posdef": case_not_posdef()}


def load_golden(path: str = GOLDEN) -> dict:
    return R.load_golden(path)
