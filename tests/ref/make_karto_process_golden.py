"""Writes tests/golden/karto_process_cases.npz: what the literal transcription tests/ref/karto_process_plain.py produces
for the directed worlds of karto_process_cases.py -- per world every output of one intake -> apply -> advance round
(records, compacted arrays, counts, pools, advance records, graph states), and the two rounds of the moved-pose
sequence.  Recorded results only: the worlds themselves are rebuilt from karto_process_cases.py.  Run from the
repository root: python tests/ref/make_karto_process_golden.py"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import karto_process_cases as K  # noqa: E402
import karto_process_plain as P  # noqa: E402
import karto_process_ref as R  # noqa: E402

STEP_KEYS = ("rec", "pool_poses", "adv", "states")


def rounds(impl) -> dict:
    """name -> the step dict of every directed round through `impl`."""
    out = {name: K.step(impl, w) for name, w in K.directed_worlds().items()}
    w, edit, cands = K.moved_sequence()
    out["moved_1"] = K.step(impl, w, edit)
    out["moved_2"] = K.step(impl, K.next_world(w, out["moved_1"], cands))
    return out


def pack(steps: dict) -> dict:
    out = {"names": np.asarray(list(steps))}
    for name, s in steps.items():
        for k in R.OUTPUT_KEYS:
            out[f"{name}/intake/{k}"] = s["intake"][k]
        for k in STEP_KEYS:
            out[f"{name}/{k}"] = s[k]
    return out


def load(path: str = R.GOLDEN) -> dict:
    z = np.load(path)
    steps = {}
    for name in [str(s) for s in z["names"]]:
        s = {k: z[f"{name}/{k}"] for k in STEP_KEYS}
        s["intake"] = {k: z[f"{name}/intake/{k}"] for k in R.OUTPUT_KEYS}
        steps[name] = s
    return steps


if __name__ == "__main__":
    np.savez_compressed(R.GOLDEN, **pack(rounds(P)))
    print(R.GOLDEN, os.path.getsize(R.GOLDEN), "bytes")
