"""Write tests/golden/karto_grid_cases.npz: the inputs of the small fixture cases (karto_grid_ref.golden_cases)
and what the CPU restatement (tests/ref/karto_grid_ref.c) gives for them -- offset and the pass / hits / state /
ros planes.  tests/test_karto_grid_cpu.py replays the restatement against the file, so a silent change of the
restatement shows up; tests/test_karto_grid_gpu.py runs the same cases on the device.  Numeric arrays only.

    python tests/ref/make_karto_grid_golden.py [output.npz]
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import karto_grid_ref as R  # noqa: E402


def main(path: str) -> None:
    cases = {name: (c, R.create_from_scans(c)) for name, c in R.golden_cases().items()}
    np.savez_compressed(path, **R.pack_golden(cases))
    for name, (c, e) in cases.items():
        print(f"{name:15s} {e['width']:4d} x {e['height']:4d}  pass {int(e['pass'].sum()):7d} hits {int(e['hits'].sum()):5d} "
              f"occupied {int((e['state'] == 100).sum()):5d} free {int((e['state'] == 255).sum()):6d}")
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else R.GOLDEN)
