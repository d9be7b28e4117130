"""cnmfe_mex('peel_open_residual_ds') through the mock MEX runtime (tests/mex_stub, the harness of tests/test_gpu_mex_gateway.py): fit, residual, the
down-sampled residual session's open with its nout variants, one extract / apply on the low-resolution grid and the close must give what the ctypes path
(Engine.peel_open_residual_ds) gives on the same library -- EQUAL arrays: the gateway only marshals (sparse double -> CSC of floats, 1-based seed -> 0-based, the
boxes clipped at the low-resolution grid, float images -> double) -- and the library's refusals come back as errors with its text."""
import os
import sys

import numpy as np
import pytest
import scipy.sparse as sp

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

pytestmark = pytest.mark.gpu


def test_the_gateway_command_gives_the_ctypes_results():
    import residual_ds_cases as dc
    from test_gpu_mex_gateway import Mex, _Geometry
    from cnmf_e_amd.engine import Engine
    from cnmf_e_amd.sources2d import PatchedVideo, seed_psf
    c = dc.CASES["B"]
    f, Y, A0, C0 = dc.inputs("B")
    d1, d2 = c["dims"]
    T, r, ssub, tsub = c["T"], c["r"], c["ssub"], c["tsub"]
    g = int(round(c["gSiz"] / ssub + 1e-9))
    psf = seed_psf(c["gSig"] / ssub, float(g), True)
    geo = PatchedVideo(d1, d2, T, c["pdims"], r, _Geometry())
    A = sp.csc_matrix(A0, dtype=np.float64)
    idx = max(geo.order, key=lambda i: int((np.asarray(abs(A[geo.patch_pix[i]]).sum(axis=0)).ravel() > 0).sum()))      # the patch most neurons of the model touch
    p, b = geo.patch_pos[idx], geo.block_pos[idx]
    nr, nc = int(p[1] - p[0] + 1), int(p[3] - p[2] + 1)
    d1s, d2s, Ts = -(-nr // ssub), -(-nc // ssub), T // tsub
    Ab = A[geo.block_pix[idx]]
    ind = np.nonzero(np.asarray(abs(Ab).sum(axis=0)).ravel() > 0)[0]
    Ab, Ap, Cb = Ab[:, ind], A[geo.patch_pix[idx]][:, ind], np.ascontiguousarray(C0[ind], dtype=np.float32)
    assert ind.size >= 1 and Ap.nnz > 0
    sr, sc = d1s // 2, d2s // 2                                           # 1-based pixel of the low-resolution grid
    blk = np.ascontiguousarray(Y[:, geo.block_pix[idx]])
    eng = Engine(0)
    try:
        eng.create_patch(0, p, b, d1, d2, T)
        eng.upload_block(0, blk)
        eng.ring_init(0, r)
        eng.fit_ring_model(0, Ab, Cb)
        eng.residual(0, Ab, Cb)
        ref_open = eng.peel_open_residual_ds(0, ssub, tsub, Ap, Cb, psf, want_video=True)
        corr, ai, ci, st = eng.peel_extract(0, sr - 1, sc - 1, g)
        s0, s1, t0, t1 = eng.peel_box(d1s, d2s, sr - 1, sc - 1, 2 * g)
        r0, r1, c0, c1 = eng.peel_box(d1s, d2s, sr - 1, sc - 1, g)
        Hai = np.zeros((s1 - s0, t1 - t0)); Hai[r0 - s0:r1 - s0, c0 - t0:c1 - t0] = ai
        ref_apply = eng.peel_apply(0, sr - 1, sc - 1, g, ai, Hai, np.nan_to_num(ci), 3.0, 5.0, 0.3)
        eng.peel_close(0)
    finally:
        eng.close()
    mex = Mex()
    h = float(mex("create", 0, nout=1)[0, 0])
    try:
        mex("patch", h, 1.0, p.astype(np.float64), b.astype(np.float64), d1, d2, T)
        mex("upload", h, 1.0, np.ascontiguousarray(blk.T), 0)
        mex("ring_init", h, 1.0, r, np.zeros((0, 0)))
        Cd = Cb.astype(np.float64)
        with pytest.raises(RuntimeError, match="has not been run"):
            mex("peel_open_residual_ds", h, 1.0, ssub, tsub, Ap, Cd, psf, nout=3)        # no resident residual
        mex("fit_ring", h, 1.0, Ab, Cd, 1, nout=1)
        mex("residual", h, 1.0, Ab, Cd)
        with pytest.raises(RuntimeError, match="ssub = 9"):
            mex("peel_open_residual_ds", h, 1.0, 9, 1, Ap, Cd, psf, nout=3)
        with pytest.raises(RuntimeError, match="tsub = 0"):
            mex("peel_open_residual_ds", h, 1.0, 2, 0, Ap, Cd, psf, nout=3)
        with pytest.raises(RuntimeError, match="at least 64"):
            mex("peel_open_residual_ds", h, 1.0, 2, 7, Ap, Cd, psf, nout=3)
        with pytest.raises(RuntimeError, match="8 inputs"):
            mex("peel_open_residual_ds", h, 1.0, 2, 2, Ap, Cd, nout=3)
        cn1 = mex("peel_open_residual_ds", h, 1.0, ssub, tsub, Ap, Cd, psf, nout=1)       # the refused calls left the residual and no session
        mex("peel_close", h, 1.0)
        mex("residual", h, 1.0, Ab, Cd)
        cn3, pnr3, sn3 = mex("peel_open_residual_ds", h, 1.0, ssub, tsub, Ap, Cd, psf, nout=3)
        mex("peel_close", h, 1.0)
        mex("residual", h, 1.0, Ab, Cd)
        cn, pnr, sn, yds = mex("peel_open_residual_ds", h, 1.0, ssub, tsub, Ap, Cd, psf, nout=4)
        assert cn.shape == (d1s, d2s) and cn.dtype == np.float64 and yds.shape == (d1s * d2s, Ts) and yds.dtype == np.float32
        for got, ref in zip((cn, pnr, sn), ref_open[:3]):
            assert np.array_equal(got.reshape(-1, order="F"), ref.astype(np.float64))
        assert np.array_equal(cn1, cn) and np.array_equal(cn3, cn) and np.array_equal(pnr3, pnr) and np.array_equal(sn3, sn)
        assert np.array_equal(yds.T, ref_open[3])
        with pytest.raises(RuntimeError, match="already has an open peel session"):
            mex("peel_open_residual_ds", h, 1.0, ssub, tsub, Ap, Cd, psf, nout=3)
        with pytest.raises(RuntimeError, match="outside the %d x %d session" % (d1s, d2s)):
            mex("peel_extract", h, 1.0, d1s + 1, sc, g, nout=4)           # inside the patch, outside the low-resolution grid
        corr_m, ai_m, ci_m, st_m = mex("peel_extract", h, 1.0, sr, sc, g, nout=4)
        assert ci_m.shape == (1, Ts)
        assert np.array_equal(corr_m, corr, equal_nan=True) and np.array_equal(ai_m, ai) and np.array_equal(ci_m.ravel(), ci, equal_nan=True)
        pnr_m, cn_m = mex("peel_apply", h, 1.0, sr, sc, g, ai, Hai, np.nan_to_num(ci), 3.0, 5.0, 0.3, nout=2)
        assert np.array_equal(pnr_m, ref_apply[0].astype(np.float64)) and np.array_equal(cn_m, ref_apply[1].astype(np.float64))
        mex("peel_close", h, 1.0)
        with pytest.raises(RuntimeError, match="no open peel session"):
            mex("peel_close", h, 1.0)
    finally:
        mex("destroy", h)
