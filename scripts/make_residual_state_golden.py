"""Writes tests/golden/residual_state_parent.npz: what the sequences of tests/residual_state_cases.py give with the build in use, for
tests/test_gpu_residual_state.py to compare a later build with, bit for bit and launch for launch.  Run ONCE, on the GPU, with the library of the commit the
comparison is against (the one before the residual's bookkeeping moved into ResidualState / residual_plan.hpp):

    CNMFE_LIB=/path/to/that/libcnmfe_hip.so python scripts/make_residual_state_golden.py --commit <hash> [--out FILE]

Only options that library knows are set.  `commit` records what wrote the file."""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--commit", required=True)
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "residual_state_parent.npz"))
    a = ap.parse_args()
    import residual_state_cases as rc
    from cnmf_e_amd import _lib
    out = {"commit": np.array(a.commit), "library": np.array(os.path.basename(_lib.LIB_PATH))}
    for name in rc.CASES:
        arrays = rc.run_case(name)
        for k, v in arrays.items():
            out["%s/%s" % (name, k)] = v
        print("%-20s %3d arrays, %7d bytes; %s" % (name, len(arrays), sum(v.nbytes for v in arrays.values()),
                                                    dict(zip(arrays["kernels"].tolist(), arrays["calls"].tolist()))), flush=True)
    np.savez_compressed(a.out, **out)
    print("wrote %s (%d bytes) for commit %s" % (a.out, os.path.getsize(a.out), a.commit))


if __name__ == "__main__":
    main()
