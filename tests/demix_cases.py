"""What the tests of orderROIs / demixed_frames / show_demixed_video share (tests/test_demix_oracle.py checks the fixture on the CPU, tests/test_gpu_demix.py and
tests/test_gpu_demix_mex.py run it on the engine): the recording of tests/df_cases.py -- 44 x 40 pixels, T = 203 (T % 4 = 3), six neurons, 2 x 2 patches of [22, 20]
with their halo, ring radius 5 (10 with bg_ssub = 2) -- after one background + spatial + temporal iteration of the oracle, plus

  halo_neuron()      a 3 x 3 footprint that lies in patch (1, 0) only, inside the halo of patch (0, 0): in (0, 0)'s block, with an EMPTY column on (0, 0)'s patch rows
  tie_nan_traces()   C, C_raw whose SNRs hold a tie (two identical rows) and a NaN (a constant row with C_raw = C: 0 / 0)

FRAME_RANGE / KT are the displayed frames of the panel comparison: the first is not a multiple of 4 (0-based 5), the last is frame T."""
import numpy as np
import scipy.sparse as sp

import df_cases
from df_cases import D1, D2, T, K, PATCH, radius, recording      # noqa: F401  (re-exported)

FRAME_RANGE, KT = (6, 203), 3
AMP_AC = 60.0                       # a fixed amplitude for the panel comparisons (the default is tested on its own)
MIXED_MARGIN = 0.05                 # distance to a rounding boundary beyond which `mixed` must equal the oracle's
ORDER_MARGIN = 1e-4                 # relative gap between neighbouring criteria the order tests need


def frames():
    """the displayed frames, 0-based"""
    return np.arange(FRAME_RANGE[0] - 1, FRAME_RANGE[1], KT)


def colors(K_):
    """K x 3 colours: the six colours of MATLAB's prism map in turn (red, orange, yellow, green, blue, violet), as float32"""
    six = np.array([[1, 0, 0], [1, 0.5, 0], [1, 1, 0], [0, 1, 0], [0, 0, 1], [2.0 / 3.0, 0, 1]], dtype=np.float32)
    return six[np.arange(K_) % 6]


def oracle_state(bg_ssub=1, deconv=False):
    """the oracle after one iteration on the recording (deconv: with the default deconvolution, as options.deconv_flag)"""
    import cnmfe_oracle as orc
    f, Y = df_cases.recording()
    r = radius(bg_ssub)
    o = orc.OracleSources2D(Y.T.reshape(D1, D2, T, order="F"), D1, D2, T, PATCH, r, f.A_init.astype(np.float32), f.C_init, f.sn, maxIter=3, bg_ssub=bg_ssub,
                            deconv_options={} if deconv else None)
    for step in ("update_background_parallel", "update_spatial_parallel", "update_temporal_parallel"):
        getattr(o, step)()
    return f, Y, o


def halo_neuron():
    """(column d x 1 float32 CSC, trace T float32): rows 23 .. 25, columns 2 .. 4 (0-based) -- patch (1, 0) starts at row 22, the halo of patch (0, 0) reaches row 26"""
    img = np.zeros((D1, D2), dtype=np.float32)
    img[23:26, 2:5] = np.array([[0.5, 1.0, 0.5], [1.0, 2.0, 1.0], [0.5, 1.0, 0.5]], dtype=np.float32)
    t = np.arange(T, dtype=np.float32)
    return sp.csc_matrix(img.reshape(-1, 1, order="F")), (3.0 + 2.0 * np.sin(t / 7.0)).astype(np.float32)


def tie_nan_traces(seed=2):
    """(C, C_raw) of six traces, float32: rows 1 and 4 are identical in both matrices (a tie), row 2 is constant with C_raw = C (var / var = 0 / 0 = NaN), row 5 has
    C_raw = C but is not constant (x / 0 = Inf: first after the NaN in a descending sort)"""
    rng = np.random.default_rng(seed)
    C = (rng.random((6, T)) * np.array([[4.0], [9.0], [1.0], [6.0], [9.0], [2.0]])).astype(np.float32)
    R = (C + (rng.standard_normal((6, T)) * np.array([[0.5], [0.7], [0.0], [0.2], [0.7], [0.0]])).astype(np.float32)).astype(np.float32)
    C[4], R[4] = C[1], R[1]
    C[2] = np.float32(1.25); R[2] = C[2]
    R[5] = C[5]
    return C, R
