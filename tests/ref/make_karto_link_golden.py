"""Writes tests/golden/karto_link_cases.npz: the directed cases' inputs (poses, matcher and search results, params)
and what the literal transcription tests/ref/karto_link_plain.py produces for them -- per stage-1 world the link
records, the job outputs and the pool poses after the call; per loop world the coarse matches that go to the fine
match and each slot's closing chain.  Data only.  Run from the repository root:
python tests/ref/make_karto_link_golden.py"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import karto_link_cases as K  # noqa: E402
import karto_link_plain as P  # noqa: E402
import karto_link_ref as R  # noqa: E402

PARAM_KEYS = ("link_match_minimum_response_fine", "loop_match_minimum_response_coarse",
              "loop_match_maximum_variance_coarse", "loop_match_minimum_response_fine")
WORLD_KEYS = ("jobs", "pool_poses", "seq", "running", "near", "near_source", "near_chains")
LOOP_KEYS = ("coarse", "source", "query", "base_begin", "base_index", "loop_chains", "pool_ranges", "fine_response")
LOOP_INTS = ("count", "capacity", "base_capacity", "tmp_first", "n_readings", "pool_scans")


def plain_loop(lw: dict):
    """The transcription's pass over every slot: (the coarse matches that go to the fine match, in order; per slot the
    closing chain or -1).  Capacity is the library's, not the reference's: the golden is taken uncut."""
    fine_of, closing = [], []
    m = 0
    for s in range(lw["count"]):
        n = int(np.sum(lw["source"]["slot"] == s))
        chains = [(lw["coarse"][m + k], {"response": lw["fine_response"][m + k]}) for k in range(n)]
        matched, closed = P.try_close_loop(lw["params"], chains)
        fine_of.extend(m + k for k in matched)
        closing.append(closed)
        m += n
    return np.asarray(fine_of, np.int32), np.asarray(closing, np.int32)


def pack(stage1: dict, loops: dict) -> dict:
    out = {"stage1_names": np.asarray(list(stage1)), "loop_names": np.asarray(list(loops))}
    for name, w in stage1.items():
        out[f"{name}/params"] = np.asarray([w["params"][k] for k in PARAM_KEYS])
        out[f"{name}/ints"] = np.asarray([w["max_links"], w["flags"]], np.int32)
        for k in WORLD_KEYS:
            out[f"{name}/{k}"] = w[k]
        links, jo, pool = P.add_edges(w)
        out[f"{name}/want_links"], out[f"{name}/want_out"], out[f"{name}/want_pool"] = links, jo, pool
    for name, lw in loops.items():
        out[f"{name}/params"] = np.asarray([lw["params"][k] for k in PARAM_KEYS])
        out[f"{name}/ints"] = np.asarray([lw[k] for k in LOOP_INTS], np.int32)
        for k in LOOP_KEYS:
            out[f"{name}/{k}"] = lw[k]
        out[f"{name}/want_fine_of"], out[f"{name}/want_closing"] = plain_loop(lw)
    return out


def load(path: str = R.GOLDEN):
    """({name: (world, want_links, want_out, want_pool)}, {name: (loop world, want_fine_of, want_closing)})."""
    z = np.load(path)
    stage1, loops = {}, {}
    for name in [str(s) for s in z["stage1_names"]]:
        w = {k: z[f"{name}/{k}"] for k in WORLD_KEYS}
        w["params"] = {k: float(v) for k, v in zip(PARAM_KEYS, z[f"{name}/params"])}
        w["max_links"], w["flags"] = (int(v) for v in z[f"{name}/ints"])
        stage1[name] = (w, z[f"{name}/want_links"], z[f"{name}/want_out"], z[f"{name}/want_pool"])
    for name in [str(s) for s in z["loop_names"]]:
        lw = {k: z[f"{name}/{k}"] for k in LOOP_KEYS}
        lw["params"] = {k: float(v) for k, v in zip(PARAM_KEYS, z[f"{name}/params"])}
        lw.update({k: int(v) for k, v in zip(LOOP_INTS, z[f"{name}/ints"])})
        loops[name] = (lw, z[f"{name}/want_fine_of"], z[f"{name}/want_closing"])
    return stage1, loops


if __name__ == "__main__":
    np.savez_compressed(R.GOLDEN, **pack(K.stage1_cases(), K.loop_cases()))
    print(R.GOLDEN, os.path.getsize(R.GOLDEN), "bytes")
