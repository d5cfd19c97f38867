"""Writes tests/golden/karto_loop_cases.npz: the directed cases' inputs and what the literal transcription
tests/ref/karto_loop_plain.py produces for them -- reference positions and, per query, the two near-linked lists, the
loop chains and the near chains.  Run from the repository root: python tests/ref/make_karto_loop_golden.py"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import karto_loop_cases as K  # noqa: E402
import karto_loop_plain as P  # noqa: E402
import karto_loop_ref as R  # noqa: E402

LASER_KEYS = ("minimum_angle", "angular_resolution", "minimum_range", "range_threshold", "n_readings")
PARAM_KEYS = ("link_scan_maximum_distance", "loop_search_maximum_distance", "loop_match_minimum_chain_size",
              "use_scan_barycenter")


def pack(cases: dict) -> dict:
    out = {"names": np.asarray(list(cases))}
    for name, c in cases.items():
        out[f"{name}/laser"] = np.asarray([float(c["laser"][k]) for k in LASER_KEYS])
        out[f"{name}/params"] = np.asarray([float(c["params"][k]) for k in PARAM_KEYS])
        for k in ("ranges", "poses", "ends", "queries"):
            out[f"{name}/{k}"] = c[k]
        out[f"{name}/reference"] = np.asarray(
            [P.barycenter(c["laser"], c["params"]["use_scan_barycenter"], r, po) for r, po in zip(c["ranges"], c["poses"])],
            np.float64).reshape(-1, 2)
        for qi, q in enumerate(c["queries"]):
            w = P.search_case(c, q)
            out[f"{name}/q{qi}/near_link"] = np.asarray(w["near_link"], np.int32)
            out[f"{name}/q{qi}/near_loop"] = np.asarray(w["near_loop"], np.int32)
            out[f"{name}/q{qi}/loop_chains"] = np.asarray(w["loop_chains"], np.int32).reshape(-1, 3)
            out[f"{name}/q{qi}/near_chains"] = np.asarray(w["near_chains"], np.int32).reshape(-1, 4)
    return out


def load(path: str = R.GOLDEN) -> dict:
    """name -> (case, reference [n, 2], [per query dict of lists])."""
    z = np.load(path)
    cases = {}
    for name in [str(s) for s in z["names"]]:
        las = {k: float(v) for k, v in zip(LASER_KEYS, z[f"{name}/laser"])}
        las["n_readings"] = int(las["n_readings"])
        prm = {k: float(v) for k, v in zip(PARAM_KEYS, z[f"{name}/params"])}
        prm["loop_match_minimum_chain_size"] = int(prm["loop_match_minimum_chain_size"])
        prm["use_scan_barycenter"] = int(prm["use_scan_barycenter"])
        c = {"laser": las, "params": prm}
        for k in ("ranges", "poses", "ends", "queries"):
            c[k] = z[f"{name}/{k}"]
        want = [{k: z[f"{name}/q{qi}/{k}"] for k in R.LIST_KEYS} for qi in range(len(c["queries"]))]
        cases[name] = (c, z[f"{name}/reference"], want)
    return cases


if __name__ == "__main__":
    np.savez_compressed(R.GOLDEN, **pack(K.directed_cases()))
    print(R.GOLDEN, os.path.getsize(R.GOLDEN), "bytes")
