"""Writes tests/golden/ring_solve_sparse_parent.npz: the ring weights of the fits of tests/solve_sparse_cases.py as the build in use computes them, for
tests/test_gpu_solve_sparse.py to compare a later build with.  Run ONCE, on the GPU, with the library of the commit the comparison is against -- a build
that applies every footprint correction to every tile:

    CNMFE_LIB=/path/to/that/libcnmfe_hip.so python scripts/make_solve_sparse_golden.py --commit <hash> [--out FILE]

Per ring radius and fit the pixel rows of solve_sparse_cases.sample_rows are kept as uint32 (the bits of the float32 weights), with max |W| of the whole fit;
`commit` records what wrote them.  Both solve kernels (solve_staged = 1 and 0) must give the same bits here, or nothing is written."""
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
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "ring_solve_sparse_parent.npz"))
    a = ap.parse_args()
    import solve_sparse_cases as sc
    from cnmf_e_amd import _lib
    from cnmf_e_amd.engine import Engine
    from cnmf_e_amd.sources2d import PatchedVideo
    out = {"commit": np.array(a.commit), "library": np.array(os.path.basename(_lib.LIB_PATH))}
    for r in sc.RADII:
        Y, fits = sc.make_inputs(r)
        rows = sc.sample_rows(r)
        out["r%d_rows" % r] = rows.astype(np.int32)
        kept = {}
        for staged in (1, 0):
            eng = Engine(0)
            try:
                eng.set_option("solve_staged", staged); eng.set_option("solve_inv", 0)
                video = PatchedVideo(sc.D1, sc.D2, sc.T, [sc.D1, sc.D2], r, eng)
                video.upload_from_full(Y)
                for k, (W, info, before) in enumerate(sc.run_fits(eng, r, fits)):
                    assert info["first_run"] == (k == 0) and np.all(np.isfinite(W.data))
                    assert before is None or info["pmax"] == before, (r, k, info["pmax"], before)
                    bits = sc.sampled_bits(W, rows)
                    if staged:
                        kept[k] = bits
                        out["r%d_fit%d" % (r, k)] = bits
                        out["r%d_fit%d_maxabs" % (r, k)] = np.float32(np.abs(W.data).max())
                        print("radius %2d fit %d: %d weights kept, max |W| %.4f, pmax %d, active %d" % (r, k, bits.size, np.abs(W.data).max(), info["pmax"], info["n_active"]))
                    else:
                        assert np.array_equal(bits, kept[k]), "radius %d fit %d: solve_staged 0 and 1 differ in this build" % (r, k)
            finally:
                eng.close()
    np.savez_compressed(a.out, **out)
    print("wrote %s (%d bytes) for commit %s" % (a.out, os.path.getsize(a.out), a.commit))


if __name__ == "__main__":
    main()
