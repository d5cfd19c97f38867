"""Write tests/golden/undistort_cases.npz: the inputs of the fixture cases (undistort_ref.golden_specs, 360
beams) and what the CPU restatement (tests/ref/undistort_ref.c) gives for them -- cloud, DataContainer points,
count, origo, status.  tests/test_undistort_cpu.py replays the restatement against the file, so a silent change
of the restatement shows up; tests/test_undistort_gpu.py runs the same cases on the device.

    python tests/ref/make_undistort_golden.py [output.npz]
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import undistort_ref as R  # noqa: E402


def main(path: str) -> None:
    cases = {}
    for name, kw in R.golden_specs():
        c = R.make_case(R.GOLDEN_N, **kw)
        cases[name] = (c, R.correct(c))
    np.savez_compressed(path, **R.pack_golden(cases))
    for name, (c, e) in cases.items():
        print(f"{name:12s} status {e['status']} points {e['n']:4d} NaNs {int(np.isnan(e['cloud']).sum())}")
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else R.GOLDEN)
