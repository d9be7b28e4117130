"""The fits of tests/test_gpu_solve_valu.py and of scripts/make_solve_golden.py (which recorded tests/golden/ring_solve_w_parent.npz with them): two successive
ring fits of a 48 x 48 patch, T = 300, K = 8 seeded footprints, at ring radii that instantiate every tile count NT = 1 .. 6 of the packed solve kernels.  At 48 x 48 the
radius-15 case has full rings (centres 15 .. 32) and rings cut by the border of the field of view."""
import numpy as np

D1, D2, T, K, SEED = 48, 48, 300, 8, 17
RADII = (2, 3, 5, 8, 10, 12, 15)              # (2 is there for NT = 1)  p = 16, 20, 40, 56, 68, 80, 96 ring pixels -> NT = 1, 2, 3, 4, 5, 5, 6 tiles of 16
NROWS, ROW_SEED = 128, 20260              # the pixel rows of W the fixture keeps


def ring_tiles(r):
    import os
    import sys
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "oracle"))
    import cnmfe_oracle as orc
    rs, _ = orc.get_nhood(r, None)
    return (len(rs) + 15) // 16


def sample_rows():
    return np.sort(np.random.default_rng(ROW_SEED).choice(D1 * D2, size=NROWS, replace=False))


def make_inputs():
    """the video (T x d, float32) and the two fits' (A, C): the blurred start, then the truth"""
    from cnmf_e_amd import synth
    f = synth.make_factors(D1, D2, T, K, SEED, gSig=2.0, gSiz=9, min_sep=5)
    Y = synth.make_video(f, np.float32)
    fits = [(f.A_init.tocsc().astype(np.float32), np.ascontiguousarray(f.C_init, dtype=np.float32)),
            (f.A_true.tocsc().astype(np.float32), np.ascontiguousarray(f.C_true, dtype=np.float32))]
    return Y, fits


def run_fits(eng, video, r, fits, pid=0):
    """ring_init + the fits; per fit (W as CSR, info of the fit)"""
    eng.ring_init(pid, r)
    out = []
    for A, C in fits:
        _, info = eng.fit_ring_model(pid, A, C)
        out.append((eng.ring_csr(pid), info))
    return out


def sampled_bits(W, rows):
    """the stored weights of the sampled pixel rows, as uint32"""
    return np.ascontiguousarray(W[rows].data, dtype=np.float32).view(np.uint32)


def crowded_inputs():
    """twelve footprints on a circle of radius 15 around pixel (24, 24): that pixel's radius-15 ring meets all of them -- more than the eight neurons a staging
    round of the packed solve kernels holds (RSP_NS), so a second round runs under the live tiles"""
    from cnmf_e_amd import synth
    f = synth.make_factors(D1, D2, T, 12, SEED + 1, gSig=1.5, gSiz=7, min_sep=3)
    ang = 2 * np.pi * np.arange(12) / 12
    centres = [(24 + 15 * np.cos(a), 24 + 15 * np.sin(a)) for a in ang]
    amp = np.random.default_rng(SEED).uniform(0.5, 1.5, 12)
    A = synth._footprints(D1, D2, centres, amp, 1.5, 5).tocsc().astype(np.float32)
    f.A_true = A; f.A_init = A
    Y = synth.make_video(f, np.float32)
    return Y, A, np.ascontiguousarray(f.C_init, dtype=np.float32)
