"""The recording and the (df_prctile, df_window) settings the dF/F tests share (tests/test_df_oracle.py checks the fixture on the CPU, tests/test_gpu_dff.py and
tests/test_gpu_dff_mex.py run it on the engine): 44 x 40 pixels, T = 203 (T % 4 = 3), six neurons, 2 x 2 patches of [22, 20], ring radius 5 (10 with bg_ssub = 2),
the state after one background + spatial + temporal iteration -- the recipe of tests/test_gpu_parity.py::test_reconstruct_background_parity.

SEED is that test's: the first seed tried on the CPU satisfied what test_df_oracle.test_fixture_is_well_conditioned asks (synth.make_video's background puts every
baseline at hundreds of counts) -- every neuron's baseline is far from zero for every setting below, and at least one neuron stores pixels in two patches, so the
cross-patch accumulation is exercised.  A change of seed has to pass that test first."""
import numpy as np

import cnmfe_oracle as orc
from cnmf_e_amd import synth

D1, D2, T, K, PATCH, SEED = 44, 40, 203, 6, [22, 20], 23
E2E_SETTINGS = [(50, None), (20, None), (50, 51), (20, 50)]                  # (df_prctile, df_window) of the end-to-end comparison


def radius(bg_ssub):
    return 5 if bg_ssub == 1 else 10


def recording(seed=SEED):
    f = synth.make_factors(D1, D2, T, K, seed, gSig=1.5, gSiz=7, min_sep=5)
    return f, synth.make_video(f, np.float32)


def oracle_after_one_iteration(f, Y, bg_ssub=1):
    r = radius(bg_ssub)
    o = orc.OracleSources2D(Y.T.reshape(D1, D2, T, order="F"), D1, D2, T, PATCH, r, f.A_init.astype(np.float32), f.C_init, f.sn, maxIter=3, bg_ssub=bg_ssub)
    for step in ("update_background_parallel", "update_spatial_parallel", "update_temporal_parallel"):
        getattr(o, step)()
    return o


def patches_of_neurons(A):
    """per neuron the set of [22, 20] patches that hold one of its stored pixels"""
    from cnmf_e_amd.sources2d import distribute_geometry
    (nr, nc), pp, _ = distribute_geometry(D1, D2, PATCH, radius(1))
    A = A.tocsc()
    out = []
    for k in range(A.shape[1]):
        rows = A.indices[A.indptr[k]:A.indptr[k + 1]][A.data[A.indptr[k]:A.indptr[k + 1]] != 0]
        r_, c_ = rows % D1 + 1, rows // D1 + 1
        out.append({(m, n) for m in range(nr) for n in range(nc)
                    if np.any((r_ >= pp[(m, n)][0]) & (r_ <= pp[(m, n)][1]) & (c_ >= pp[(m, n)][2]) & (c_ <= pp[(m, n)][3]))})
    return out
