"""cnmfe_mex('seed_images_ds', ...) and cnmfe_mex('peel_open_ds', ...) through the mock MEX runtime (tests/mex_stub, the harness of
tests/test_gpu_mex_gateway.py): the commands the twin @Sources2D/correlation_pnr_parallel.m and a MATLAB host of the down-sampled initialisation issue per
patch must give what the Python engine's seed_images_ds / peel_open_ds give on the same library -- EQUAL arrays: the gateway only marshals."""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

pytestmark = pytest.mark.gpu


def test_the_gateway_commands_give_the_python_engines_results():
    from test_gpu_mex_gateway import Mex
    import ds_cases as dc
    from cnmf_e_amd.engine import Engine
    from cnmf_e_amd.sources2d import PatchedVideo, seed_psf, bspline_basis
    c = dc.CASES["S"]
    _, Y = dc.inputs("S")
    d1, d2 = c["dims"]
    T, r, ssub, tsub, nk = c["T"], c["r"], c["ssub"], c["tsub"], c["nk"]
    d1s, d2s, Ts = -(-d1 // ssub), -(-d2 // ssub), T // tsub
    psf = seed_psf(c["gSig"] / ssub, np.ceil(c["gSiz"] / ssub), True)
    Qs = np.linalg.qr(bspline_basis(Ts, nk))[0]
    Qpre = np.linalg.qr(bspline_basis(T, nk))[0]
    eng = Engine(0)
    try:
        video = PatchedVideo(d1, d2, T, [d1, d2], r, eng)
        video.upload_from_full(Y)
        cn_ref, pnr_ref = eng.seed_images_ds(0, ssub, tsub, psf, T, Qs)
        cn2_ref, pnr2_ref, sn_ref, yds_ref = eng.peel_open_ds(0, ssub, tsub, psf, T, Qpre, want_video=True)
        ex_ref = eng.peel_extract(0, 10, 9, 7)
        eng.peel_close(0)
    finally:
        eng.close()
    mex = Mex()
    h = float(mex("create", 0, nout=1)[0, 0])
    try:
        pos = np.array([1, d1, 1, d2], dtype=np.float64)
        mex("patch", h, 1.0, pos, pos, d1, d2, T)
        mex("upload", h, 1.0, np.ascontiguousarray(Y.T), 0)
        cn, pnr = mex("seed_images_ds", h, 1.0, ssub, tsub, psf, T, Qs, nout=2)
        assert cn.shape == (d1s, d2s) and cn.dtype == np.float64 and pnr.shape == cn.shape
        assert np.array_equal(cn.reshape(-1, order="F"), cn_ref) and np.array_equal(pnr.reshape(-1, order="F"), pnr_ref)
        cn2, pnr2, sn, yds = mex("peel_open_ds", h, 1.0, ssub, tsub, psf, T, Qpre, nout=4)
        assert yds.shape == (d1s * d2s, Ts) and yds.dtype == np.float32 and np.array_equal(yds.T, yds_ref)
        assert np.array_equal(cn2.reshape(-1, order="F"), cn2_ref) and np.array_equal(pnr2.reshape(-1, order="F"), pnr2_ref)
        assert np.array_equal(sn.reshape(-1, order="F"), sn_ref)
        corr, ai, ci, st = mex("peel_extract", h, 1.0, 11, 10, 7, nout=4)                  # 1-based on the low-resolution grid
        assert ci.shape == (1, Ts) and np.array_equal(corr, ex_ref[0], equal_nan=True) and np.array_equal(ai, ex_ref[1]) and np.array_equal(ci[0], ex_ref[2])
        with pytest.raises(RuntimeError, match="outside the %d x %d session" % (d1s, d2s)):
            mex("peel_extract", h, 1.0, d1s + 1, 1, 7, nout=4)
        mex("peel_close", h, 1.0)
        with pytest.raises(RuntimeError, match="ssub = 9"):
            mex("seed_images_ds", h, 1.0, 9, 1, psf, T, nout=2)
        with pytest.raises(RuntimeError, match="at least 64"):
            mex("peel_open_ds", h, 1.0, 1, 10, psf, T, nout=3)
        with pytest.raises(RuntimeError, match="not created through this gateway"):
            mex("seed_images_ds", h, 99.0, 2, 2, psf, T, nout=2)
    finally:
        mex("destroy", h)
