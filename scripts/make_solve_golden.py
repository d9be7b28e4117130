"""Writes tests/golden/ring_solve_w_parent.npz: the ring weights of the fits of tests/solve_valu_cases.py as the build in use computes them, for
tests/test_gpu_solve_valu.py to compare a later build with.  Run ONCE, on the GPU, with the library of the commit the comparison is against:

    CNMFE_LIB=/path/to/that/libcnmfe_hip.so python scripts/make_solve_golden.py --commit <hash> [--out FILE]

Per ring radius and fit, a fixed, seeded sample of 128 pixel rows of W is kept as uint32 (the bits of the float32 weights), with max |W| of the whole fit;
`commit` records what wrote them (default, for the in-tree library only: git rev-parse HEAD of the working tree; with CNMFE_LIB it must be given)."""
import argparse
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--commit", default=None)
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "ring_solve_w_parent.npz"))
    a = ap.parse_args()
    if a.commit is None and os.environ.get("CNMFE_LIB"):
        ap.error("--commit is required when CNMFE_LIB selects the library: the working tree's HEAD need not be what built it")
    commit = a.commit or subprocess.run(["git", "rev-parse", "HEAD"], cwd=ROOT, capture_output=True, text=True, check=True).stdout.strip()
    import solve_valu_cases as sc
    from cnmf_e_amd import _lib
    from cnmf_e_amd.engine import Engine
    from cnmf_e_amd.sources2d import PatchedVideo
    Y, fits = sc.make_inputs()
    rows = sc.sample_rows()
    out = {"commit": np.array(commit), "rows": rows.astype(np.int32), "library": np.array(os.path.basename(_lib.LIB_PATH))}
    for r in sc.RADII:
        eng = Engine(0)
        try:
            video = PatchedVideo(sc.D1, sc.D2, sc.T, [sc.D1, sc.D2], r, eng)
            video.upload_from_full(Y)
            for k, (W, info) in enumerate(sc.run_fits(eng, video, r, fits)):
                assert info["first_run"] == (k == 0) and np.all(np.isfinite(W.data))
                out["r%d_fit%d" % (r, k)] = sc.sampled_bits(W, rows)
                out["r%d_fit%d_maxabs" % (r, k)] = np.float32(np.abs(W.data).max())
                print("radius %2d fit %d: %d weights kept, max |W| %.4f, pmax %d, active %d" % (r, k, out["r%d_fit%d" % (r, k)].size, np.abs(W.data).max(), info["pmax"], info["n_active"]))
        finally:
            eng.close()
    np.savez_compressed(a.out, **out)
    print("wrote %s (%d bytes) for commit %s" % (a.out, os.path.getsize(a.out), commit))


if __name__ == "__main__":
    main()
