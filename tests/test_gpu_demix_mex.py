"""The closing commands of the MEX gateway -- 'trace_order_stats', 'demix_frames', 'demix_frames_ssub' -- through the mock MEX runtime (tests/mex_stub, the harness
of tests/test_gpu_mex_gateway.py) against the ctypes path on the same library: EQUAL arrays, the gateway only marshals (double -> float, 1-based rows -> 0-based,
column-major colours -> row-major, the uint16 panel handed out as single)."""
import os
import sys

import numpy as np
import pytest
import scipy.sparse as sp

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

pytestmark = pytest.mark.gpu

NAMES = ("raw", "bg", "signal", "denoised", "residual")


def test_the_closing_commands_give_the_ctypes_results():
    import demix_cases as dc
    from test_gpu_mex_gateway import Mex, _Geometry
    from cnmf_e_amd.engine import Engine
    from cnmf_e_amd.sources2d import PatchedVideo
    f, Y = dc.recording()
    d1, d2, T, r, ssub = dc.D1, dc.D2, dc.T, 10, 2
    A = sp.csc_matrix(f.A_init, dtype=np.float32)
    Cm = np.ascontiguousarray(f.C_init, dtype=np.float32)
    Cr = (Cm + np.random.default_rng(3).standard_normal(Cm.shape).astype(np.float32) * 0.25).astype(np.float32)
    K = A.shape[1]
    col = dc.colors(K)
    geo = PatchedVideo(d1, d2, T, dc.PATCH, r, _Geometry())
    rng = np.random.default_rng(0)
    b0 = {idx: (rng.random(geo.block_pix[idx].size) * 3).astype(np.float32) for idx in geo.order}
    b0n = {idx: (100 + rng.random(geo.patch_pix[idx].size)).astype(np.float32) for idx in geo.order}
    frame0, stride, nf, scale = 5, dc.KT, 9, 2.0 / dc.AMP_AC * 65536.0

    def pieces(idx):
        Ab, Ap = A[geo.block_pix[idx]], A[geo.patch_pix[idx]]
        indb = np.nonzero(np.asarray(abs(Ab).sum(axis=0)).ravel() > 0)[0]
        indp = np.nonzero(np.asarray(abs(Ap).sum(axis=0)).ravel() > 0)[0]
        return Ab[:, indb], indb, Ap[:, indp], indp

    # the ctypes route: the initial ring (W = 1 / count); per patch the panels from the bound matrix, from the resident C_raw and (bg_ssub = 2) from a host matrix
    ref, ref_raw, ref_ssub = {}, {}, {}
    eng = Engine(0)
    try:
        video = PatchedVideo(d1, d2, T, dc.PATCH, r, eng)
        video.upload_from_full(Y)
        eng.traces_load(Cm, Cr)
        stats = eng.trace_order_stats()
        for idx in video.order:
            Ab, indb, Ap, indp = pieces(idx)
            pid = video.pid[idx]
            eng.ring_init(pid, r)
            eng.residual(pid, Ab if indb.size else None, Cm[indb] if indb.size else None)
            ref[idx] = eng.demix_frames(pid, b0[idx], b0n[idx], Ap, Cm, indp, col[indp], scale, frame0, stride, nf)
            ref_raw[idx] = eng.demix_frames(pid, b0[idx], b0n[idx], Ap, Cr, indp, col[indp], scale, frame0, stride, nf)
        idx = video.order[0]
        Ab, indb, Ap, indp = pieces(idx)
        pid, fit = video.pid[idx], 100
        eng.patch_derive(pid, fit, ssub, "nearest")
        eng.ring_init(fit, r // ssub)
        eng.background_ssub(pid, fit, ssub, Ab if indb.size else None, Cm[indb] if indb.size else None, b0[idx])
        ref_ssub = eng.demix_frames(pid, None, b0n[idx], Ap, np.array(Cm), indp, col[indp], scale, frame0, stride, nf)
    finally:
        eng.close()
    assert any(ref[idx]["denoised"].any() for idx in geo.order) and ref_ssub["bg"].any()

    def same(got, want, d):
        for j, name in enumerate(NAMES):
            assert got[j].dtype == np.float32 and got[j].shape == (d, nf) and np.array_equal(got[j], want[name].T), name
        assert got[5].dtype == np.float32 and got[5].shape == (d, 3 * nf)                     # colour plane m in columns m nf .. (m + 1) nf
        assert np.array_equal(got[5].reshape(d, nf, 3, order="F"), want["mixed"].transpose(2, 1, 0).astype(np.float32))

    mex = Mex()
    h = float(mex("create", 0, nout=1)[0, 0])
    try:
        pid = {idx: float(i + 1) for i, idx in enumerate(geo.order)}
        dbl = lambda a: np.asarray(a, dtype=np.float64)
        with pytest.raises(RuntimeError, match="holds no C, C_raw"):
            mex("trace_order_stats", h, K, nout=1)
        mex("traces_load", h, dbl(Cm), dbl(Cr), np.zeros((0, 0)), np.zeros((0, 0)))
        q = mex("trace_order_stats", h, K, nout=1)
        assert q.shape == (K, 7) and np.array_equal(q, stats)
        for idx in geo.order:
            Ab, indb, Ap, indp = pieces(idx)
            d = geo.patch_pix[idx].size
            mex("patch", h, pid[idx], geo.patch_pos[idx].astype(np.float64), geo.block_pos[idx].astype(np.float64), d1, d2, T)
            mex("upload", h, pid[idx], np.ascontiguousarray(Y[:, geo.block_pix[idx]].T), 0)
            mex("ring_init", h, pid[idx], r, np.zeros((0, 0)))
            tail = (dbl(col[indp]), scale, frame0, stride, nf)
            with pytest.raises(RuntimeError, match="cnmfe_residual has not been run"):
                mex("demix_frames", h, pid[idx], dbl(b0[idx]), dbl(b0n[idx]), Ap.astype(np.float64), "bound", (indp + 1).astype(np.float64), *tail, nout=6)
            mex("residual", h, pid[idx], Ab.astype(np.float64), dbl(Cm[indb]))
            with pytest.raises(RuntimeError, match="unknown source"):
                mex("demix_frames", h, pid[idx], dbl(b0[idx]), dbl(b0n[idx]), Ap.astype(np.float64), "s", (indp + 1).astype(np.float64), *tail, nout=6)
            with pytest.raises(RuntimeError, match="reach beyond"):
                mex("demix_frames", h, pid[idx], dbl(b0[idx]), dbl(b0n[idx]), Ap.astype(np.float64), "bound", (indp + 1).astype(np.float64), dbl(col[indp]), scale, T - 2, stride, nf,
                    nout=6)
            got = mex("demix_frames", h, pid[idx], dbl(b0[idx]), dbl(b0n[idx]), Ap.astype(np.float64), "bound", (indp + 1).astype(np.float64), *tail, nout=6)
            same(got, ref[idx], d)
            got = mex("demix_frames", h, pid[idx], dbl(b0[idx]), dbl(b0n[idx]), Ap.astype(np.float64), "craw", (indp + 1).astype(np.int32), *tail, nout=6)
            same(got, ref_raw[idx], d)
            got = mex("demix_frames", h, pid[idx], dbl(b0[idx]), dbl(b0n[idx]), Ap.astype(np.float64), dbl(Cm[indp]), np.zeros((0, 0)), *tail, nout=6)      # a host matrix
            same(got, ref[idx], d)
        idx = geo.order[0]
        Ab, indb, Ap, indp = pieces(idx)
        fit = 100.0
        tail = (dbl(col[indp]), scale, frame0, stride, nf)
        with pytest.raises(RuntimeError, match="cnmfe_background_ssub has not been run"):
            mex("demix_frames_ssub", h, pid[idx], dbl(b0n[idx]), Ap.astype(np.float64), dbl(Cm[indp]), np.zeros((0, 0)), *tail, nout=6)
        mex("derive", h, pid[idx], fit, ssub, "nearest")
        mex("ring_init", h, fit, r // ssub, np.zeros((0, 0)))
        mex("background_ssub", h, pid[idx], fit, ssub, Ab.astype(np.float64), dbl(Cm[indb]), dbl(b0[idx]))
        got = mex("demix_frames_ssub", h, pid[idx], dbl(b0n[idx]), Ap.astype(np.float64), dbl(Cm[indp]), np.zeros((0, 0)), *tail, nout=6)
        same(got, ref_ssub, geo.patch_pix[idx].size)
    finally:
        mex("destroy", h)
