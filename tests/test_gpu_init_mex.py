"""cnmfe_mex('peel_open' / 'peel_extract' / 'peel_apply' / 'peel_close') through the mock MEX runtime (tests/mex_stub, the harness of
tests/test_gpu_mex_gateway.py): one open / extract / apply / close on a patch must give what the ctypes path (Engine.peel_*) gives on the same library --
EQUAL arrays: the gateway only marshals (double psf -> float, 1-based seed -> 0-based, the clipped box shapes, float images -> double)."""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

pytestmark = pytest.mark.gpu


def test_the_gateway_commands_give_the_ctypes_results():
    import greedy_cases as gc
    from test_gpu_mex_gateway import Mex
    from cnmf_e_amd.engine import Engine
    from cnmf_e_amd.sources2d import PatchedVideo, seed_psf
    c = gc.CASES["A"]
    _, Y = gc.inputs("A")
    d1, d2 = c["dims"]
    T, r, g = c["T"], c["r"], c["gSiz"]
    psf = seed_psf(c["gSig"], c["gSiz"], True)
    geo = gc.geometry("A")
    idx = geo.order[0]
    p, b = geo.patch_pos[idx], geo.block_pos[idx]
    nrb, ncb = int(b[1] - b[0] + 1), int(b[3] - b[2] + 1)
    ctr = gc.oracle("A")["blocks"][idx]["center"]
    sr, sc = (int(ctr[0, 0]), int(ctr[0, 1])) if ctr.shape[0] else (nrb // 2, ncb // 2)      # 1-based block pixel
    eng = Engine(0)
    try:
        video = PatchedVideo(d1, d2, T, c["pdims"], r, eng)
        video.upload_from_full(Y)
        pid = video.pid[idx]
        ref_open = eng.peel_open(pid, psf, T)
        corr, ai, ci, st = eng.peel_extract(pid, sr - 1, sc - 1, g)
        s0, s1, t0, t1 = eng.peel_box(nrb, ncb, sr - 1, sc - 1, 2 * g)
        r0, r1, c0, c1 = eng.peel_box(nrb, ncb, sr - 1, sc - 1, g)
        Hai = np.zeros((s1 - s0, t1 - t0)); Hai[r0 - s0:r1 - s0, c0 - t0:c1 - t0] = ai
        ref_apply = eng.peel_apply(pid, sr - 1, sc - 1, g, ai, Hai, ci, 3.0, 10.0, 0.3)
        eng.peel_close(pid)
    finally:
        eng.close()
    mex = Mex()
    h = float(mex("create", 0, nout=1)[0, 0])
    try:
        mex("patch", h, 1.0, p.astype(np.float64), b.astype(np.float64), d1, d2, T)
        mex("upload", h, 1.0, np.ascontiguousarray(Y[:, geo.block_pix[idx]].T), 0)
        with pytest.raises(RuntimeError, match="no open peel session"):
            mex("peel_extract", h, 1.0, sr, sc, g, nout=4)
        cn_b, pnr_b, sn_b = mex("peel_open", h, 1.0, psf, T, np.zeros((0, 0)), nout=3)
        assert cn_b.shape == (nrb, ncb) and cn_b.dtype == np.float64
        for got, ref in zip((cn_b, pnr_b, sn_b), ref_open):
            assert np.array_equal(got.reshape(-1, order="F"), ref.astype(np.float64))
        with pytest.raises(RuntimeError, match="already has an open peel session"):
            mex("peel_open", h, 1.0, psf, T, nout=3)
        corr_m, ai_m, ci_m, st_m = mex("peel_extract", h, 1.0, sr, sc, g, nout=4)
        assert np.array_equal(corr_m, corr) and np.array_equal(ai_m, ai) and np.array_equal(ci_m.ravel(), ci)
        assert np.array_equal(st_m.ravel(), [st["max_diff"], st["std_diff"], st["norm_ci"], st["sn_ci"], st["n_hi"], st["n_lo"]])
        pnr_m, cn_m = mex("peel_apply", h, 1.0, sr, sc, g, ai, Hai, ci, 3.0, 10.0, 0.3, nout=2)
        assert np.array_equal(pnr_m, ref_apply[0].astype(np.float64)) and np.array_equal(cn_m, ref_apply[1].astype(np.float64))
        with pytest.raises(RuntimeError, match="gSiz <= 20"):
            mex("peel_extract", h, 1.0, sr, sc, 21, nout=4)
        mex("peel_close", h, 1.0)
        with pytest.raises(RuntimeError, match="no open peel session"):
            mex("peel_close", h, 1.0)
    finally:
        mex("destroy", h)
