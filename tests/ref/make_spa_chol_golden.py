"""Write tests/golden/spa_chol_cases.npz: the inputs of the named pose graphs (spa2d_chol_ref.golden_cases) and what
the direct-mode restatement (tests/ref/spa2d_chol_ref.c) gives for them -- final poses and the stats, in
spa_cases.npz's layout.  tests/test_spa_chol_cpu.py replays the restatement against the file; tests/test_spa_chol_gpu.py
runs the same cases on the device.  Numeric arrays only.

    python tests/ref/make_spa_chol_golden.py [output.npz]
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import spa2d_chol_ref as CH  # noqa: E402
import spa2d_ref as R  # noqa: E402


def main(path: str) -> None:
    cases = {}
    for name, c in CH.golden_cases().items():
        po, st = CH.compute_case(c)
        cases[name] = (c, po, st)
        print(f"{name:10s} nodes {len(c['poses']):4d} cons {len(c['ends']):4d} blocks {CH.envelope_blocks(c):5d}  status "
              f"{st['status']} lm {st['lm_iters']:3d} good {st['good_iter']:3d} rejected {st['rejected']:2d} converged "
              f"{st['converged']} cost {st['initial_cost']:.6g} -> {st['final_cost']:.6g}")
    np.savez_compressed(path, **R.pack_golden(cases))
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else CH.GOLDEN)
