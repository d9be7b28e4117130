"""Seed images beyond the 20 416 frames a trace and its Welch transform share one workgroup's LDS (k_seed_stats_long, csrc/seed.hpp), at the three frame counts
of tests/long_cases.py against the float64 oracle tests/seed_oracle.py.  Block 20 x 18: tiles of 16 + 4 rows and 16 + 2 columns, one patch, ring radius 3.

(a) PNR on every pixel, relative, of the filtered (gSig 1.5, center_psf) and detrended (nk = 3) float video through Sources2D.correlation_pnr_parallel at
    20 417 and 40 001 frames: 2e-4, the bound tests/test_gpu_edges.py::test_get_sn_of_long_recordings asserts of the same Welch estimator at these lengths.
    Cn is only checked for being finite and in [-1, 1] there: on such a video the step HY < 3 Sn cannot be compared sample by sample (most pixels have
    themselves or a neighbour within 1e-4 Sn of the threshold at these lengths).
(b) Cn on the robust pixels and PNR on every pixel, at all three counts, of the QUANTISED video Y4 = 4 rint(Y / 4) with no filter (eng.seed_images(0, None)):
    HY - median sits on a grid of spacing 4 that the threshold rarely meets.  A pixel is fragile when the oracle's margin is below 2e-3 (3 x the 2e-4 Sn
    bound x 3, rounded up) and is left out with its neighbours; at most 10 % may be left out (tests/test_long_fixtures.py recomputes the shares on the CPU).
    Cn absolute 2e-6, PNR relative 2e-4 before tightening (below); the left-out pixels must be finite and in [-1, 1]."""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import long_cases as lc

pytestmark = pytest.mark.gpu

# The bounds the Welch estimator's test gives (PNR 2e-4 relative) and tests/test_gpu_seed_images.py asserts (Cn 2e-6 absolute), tightened by the rule of
# tests/test_gpu_parity.py to 10 x the error observed on the MI355X, rounded up to one digit, where that is lower.  Observed:
#   (a) PNR relative 1.9e-6 (20 417), 1.9e-6 (40 001)                                                       -> 2e-5
#   (b) PNR relative 9.2e-8 / 9.0e-8 / 9.4e-8, Cn absolute 3.0e-8 / 3.0e-8 / 3.0e-8 (robust = all pixels)   -> 1e-6, 3e-7
#       left out 2.5 % / 0 % / 0 %
PNR_TOL = 2e-5
PNR_Q_TOL = 1e-6
CN_TOL = 3e-7


def _video(eng, Y, T):
    from cnmf_e_amd.sources2d import PatchedVideo
    d1, d2 = lc.SEED["dims"]
    video = PatchedVideo(d1, d2, T, [d1, d2], lc.SEED["r"], eng)
    video.upload_from_full(Y)
    return video


@pytest.mark.parametrize("T", lc.T_LONG[:2])
def test_pnr_of_the_filtered_detrended_video(T, observed):
    from cnmf_e_amd.sources2d import Sources2D, Options
    f, Y = lc.seed_video(T)
    eng = lc.engine()
    try:
        s = Sources2D(_video(eng, Y, T), Options(ring_radius=lc.SEED["r"], gSig=lc.SEED["gSig"], gSiz=lc.SEED["gSiz"], center_psf=True, nk=lc.SEED["nk"]),
                      f.A_init, f.C_init, f.sn)
        Cn, PNR = s.correlation_pnr_parallel()
    finally:
        eng.close()
    ref = lc.seed_oracle_pnr(T)
    e = float(np.max(np.abs(PNR - ref) / np.abs(ref)))
    observed["long_seed_pnr_%d" % T] = dict(pnr_rel=e)
    print("long seed images (filter, detrend) T = %d: PNR rel %.3e" % (T, e))
    assert np.all(np.isfinite(Cn)) and Cn.min() >= -1.0 and Cn.max() <= 1.0
    assert e <= PNR_TOL, e


@pytest.mark.parametrize("T", lc.T_LONG)
def test_quantised_video_without_filter(T, observed):
    d1, d2 = lc.SEED["dims"]
    eng = lc.engine()
    try:
        _video(eng, lc.seed_video_q(T), T)
        Cn, PNR = eng.seed_images(0, None)
    finally:
        eng.close()
    Cn = Cn.astype(np.float64).reshape(d1, d2, order="F"); PNR = PNR.astype(np.float64).reshape(d1, d2, order="F")
    Cn_o, PNR_o, robust = lc.seed_oracle_q(T)
    left = float((~robust).mean())
    e_pnr = float(np.max(np.abs(PNR - PNR_o) / np.abs(PNR_o)))
    e_cn = float(np.max(np.abs(Cn - Cn_o)[robust]))
    observed["long_seed_q_%d" % T] = dict(pnr_rel=e_pnr, cn_abs_robust=e_cn, cn_abs_all=float(np.max(np.abs(Cn - Cn_o))), left_out=left)
    print("long seed images (quantised) T = %d: PNR rel %.3e  Cn abs (robust) %.3e  (all) %.3e  left out %.2f %%" % (T, e_pnr, e_cn, float(np.max(np.abs(Cn - Cn_o))), 100 * left))
    assert left <= lc.SEED_LEFT_MAX, left
    assert np.all(np.isfinite(Cn)) and Cn.min() >= -1.0 and Cn.max() <= 1.0
    assert e_pnr <= PNR_Q_TOL, e_pnr
    assert e_cn <= CN_TOL, e_cn
