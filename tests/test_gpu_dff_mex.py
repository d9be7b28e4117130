"""The dF/F commands of the MEX gateway -- 'df_begin', 'df_add_background', 'df_add_frames', 'df_fetch', 'df_load', 'df_finish' -- through the mock MEX runtime
(tests/mex_stub, the harness of tests/test_gpu_mex_gateway.py) against the ctypes path on the same library: EQUAL arrays, the gateway only marshals (double ->
float, 1-based rows -> 0-based, row-major results -> column-major)."""
import os
import sys

import numpy as np
import pytest
import scipy.sparse as sp

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

pytestmark = pytest.mark.gpu


def test_the_df_commands_give_the_ctypes_results():
    import df_cases
    from test_gpu_mex_gateway import Mex, _Geometry
    from cnmf_e_amd.engine import Engine
    from cnmf_e_amd.sources2d import PatchedVideo
    f, Y = df_cases.recording()
    d1, d2, T, r = df_cases.D1, df_cases.D2, df_cases.T, 5
    A = sp.csc_matrix(f.A_init, dtype=np.float32)
    Cm = np.ascontiguousarray(f.C_init, dtype=np.float32)
    K = A.shape[1]
    geo = PatchedVideo(d1, d2, T, df_cases.PATCH, r, _Geometry())
    rng = np.random.default_rng(0)
    b0 = {idx: (rng.random(geo.block_pix[idx].size) * 3).astype(np.float32) for idx in geo.order}
    b0n = {idx: (100 + rng.random(geo.patch_pix[idx].size)).astype(np.float32) for idx in geo.order}
    with np.errstate(divide="ignore"):
        inv = 1.0 / np.asarray(A.astype(np.float64).power(2).sum(axis=0)).ravel()

    def pieces(idx):
        Ab, Ap = A[geo.block_pix[idx]], A[geo.patch_pix[idx]]
        indb = np.nonzero(np.asarray(abs(Ab).sum(axis=0)).ravel() > 0)[0]
        indp = np.nonzero(np.asarray(abs(Ap).sum(axis=0)).ravel() > 0)[0]
        return Ab[:, indb], indb, Ap[:, indp], indp

    # the ctypes route: the initial ring (W = 1 / count), the residual of (A, C), all four patches, a windowed percentile
    eng = Engine(0)
    try:
        video = PatchedVideo(d1, d2, T, df_cases.PATCH, r, eng)
        video.upload_from_full(Y)
        eng.bind_traces(Cm)
        eng.df_begin(K, T)
        for idx in video.order:
            Ab, indb, Ap, indp = pieces(idx)
            pid = video.pid[idx]
            eng.ring_init(pid, r)
            eng.residual(pid, Ab if indb.size else None, Cm[indb] if indb.size else None)
            eng.df_add_background(pid, b0[idx], b0n[idx], Ap, indp)
        ref_acc = eng.df_fetch()
        ref = eng.df_finish(inv, 20, 50, Cm, Cm, want_Yf=True)
    finally:
        eng.close()
    assert np.abs(ref_acc).max() > 0
    mex = Mex()
    h = float(mex("create", 0, nout=1)[0, 0])
    try:
        pid = {idx: float(i + 1) for i, idx in enumerate(geo.order)}
        d = lambda a: np.asarray(a, dtype=np.float64)
        with pytest.raises(RuntimeError, match="cnmfe_df_begin has not been called"):
            mex("df_fetch", h, nout=1)
        mex("df_begin", h, K, T)
        with pytest.raises(RuntimeError, match="is open"):
            mex("df_begin", h, K, T)
        for idx in geo.order:
            Ab, indb, Ap, indp = pieces(idx)
            mex("patch", h, pid[idx], geo.patch_pos[idx].astype(np.float64), geo.block_pos[idx].astype(np.float64), d1, d2, T)
            mex("upload", h, pid[idx], np.ascontiguousarray(Y[:, geo.block_pix[idx]].T), 0)
            mex("ring_init", h, pid[idx], r, np.zeros((0, 0)))
            with pytest.raises(RuntimeError, match="cnmfe_residual has not been run"):
                mex("df_add_background", h, pid[idx], d(b0[idx]), d(b0n[idx]), Ap.astype(np.float64), (indp + 1).astype(np.float64))
            mex("residual", h, pid[idx], Ab.astype(np.float64), d(Cm[indb]))
            with pytest.raises(RuntimeError, match="listed twice|outside"):
                mex("df_add_background", h, pid[idx], d(b0[idx]), d(b0n[idx]), Ap.astype(np.float64), np.full(indp.size, K + 1.0))
            mex("df_add_background", h, pid[idx], d(b0[idx]), d(b0n[idx]), Ap.astype(np.float64), (indp + 1).astype(np.int32))
        acc = mex("df_fetch", h, nout=1)
        assert acc.shape == (K, T) and np.array_equal(acc, ref_acc)
        mex("df_load", h, acc)
        with pytest.raises(RuntimeError, match="unknown source"):
            mex("df_finish", h, inv, 20, 50, "craww", d(Cm), nout=3)
        with pytest.raises(RuntimeError, match="df_prctile"):
            mex("df_finish", h, inv, 101, 50, d(Cm), d(Cm), nout=3)
        C_df, R_df, Df, Yf = mex("df_finish", h, inv, 20, 50, d(Cm), Cm, nout=4)
        assert C_df.dtype == np.float32 and Df.shape == (K, T)
        for got, want in zip((C_df, R_df, Df, Yf), ref):
            assert np.array_equal(got, want, equal_nan=True)
        # the accumulator is closed; a slab the caller holds, no window: Df is K x 1
        mex("df_begin", h, K, T)
        slab = np.ascontiguousarray(rng.random((d1 * d2, 16)) + 5, dtype=np.float32)
        mex("df_add_frames", h, slab, 3, A.astype(np.float64), np.arange(1, K + 1, dtype=np.float64))
        C_df, R_df, Df = mex("df_finish", h, inv, 50, np.zeros((0, 0)), d(Cm), d(Cm), nout=3)
        assert Df.shape == (K, 1) and np.all(Df == 0)                      # (16 of 203 frames hold anything: the median is 0)
    finally:
        mex("destroy", h)
    eng = Engine(0)
    try:
        eng.df_begin(K, T)
        eng.df_add_frames(slab.T, 3, A, np.arange(K))
        acc2 = eng.df_fetch()
        eng.df_close()
        want = np.zeros((K, T))
        want[:, 3:19] = np.asarray(A.astype(np.float64).T @ slab.astype(np.float64))
        assert np.abs(acc2 - want).max() <= 1e-13 * np.abs(want).max()
    finally:
        eng.close()
