"""Writes tests/golden/fit_setup_parent.npz: what the runs of tests/fit_side_cases.py give with the build in use -- sampled rows of W, b0 and the info of every
fit, A and C after the full iterations -- for tests/test_gpu_fit_side.py to compare a later build with, bit for bit.  Run ONCE, on the GPU, with the library of
the commit the comparison is against (the one before the fit's set-up moved: host-side sum(A, 2) and slot_of, tables uploaded every fit, one stream):

    CNMFE_LIB=/path/to/that/libcnmfe_hip.so python scripts/make_fit_setup_golden.py --commit <hash> [--out FILE]

Option fit_side is never set here (that library does not know it).  `commit` records what wrote the file."""
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
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "fit_setup_parent.npz"))
    a = ap.parse_args()
    import fit_side_cases as fc
    from cnmf_e_amd import _lib
    out = {"commit": np.array(a.commit), "library": np.array(os.path.basename(_lib.LIB_PATH))}
    for name in fc.CASES:
        arrays, _ = fc.run_case(name, None)
        for k, v in arrays.items():
            out["%s/%s" % (name, k)] = v
        infos = {k: v.tolist() for k, v in arrays.items() if k.endswith("_info")}
        print("%-16s %3d arrays, %7d bytes; info %s" % (name, len(arrays), sum(v.nbytes for v in arrays.values()), infos), flush=True)
    np.savez_compressed(a.out, **out)
    print("wrote %s (%d bytes) for commit %s" % (a.out, os.path.getsize(a.out), a.commit))


if __name__ == "__main__":
    main()
