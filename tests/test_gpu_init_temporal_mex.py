"""cnmfe_mex('init_temporal') through the mock MEX runtime (tests/mex_stub, the harness of tests/test_gpu_mex_gateway.py): the command must give what the ctypes
path (Engine.init_temporal) gives on the same library -- EQUAL arrays: the gateway only marshals (double sparse A -> int64 / int32 / float CSC, column-major
K x T float results -> double)."""
import os
import sys

import numpy as np
import pytest
import scipy.sparse as sp

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(os.path.dirname(HERE), "oracle"))

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("name", ["A", "B"])
def test_the_gateway_command_gives_the_ctypes_result(name):
    import init_temporal_cases as itc
    from test_gpu_mex_gateway import Mex
    from cnmf_e_amd.engine import Engine
    from cnmf_e_amd.sources2d import PatchedVideo
    c = itc.make(name)
    eng = Engine(0)
    try:
        video = PatchedVideo(c.d1, c.d2, c.T, c.pdims, c.r, eng)
        video.upload_from_full(c.Y)
        idx = video.order[0]; pid = video.pid[idx]
        p, b, bp = video.patch_pos[idx], video.block_pos[idx], video.block_pix[idx]
        eng.ring_init(pid, c.r)
        W = sp.csr_matrix(c.W[idx]); W.sort_indices()
        eng.ring_set_values(pid, W.data); eng.set_b0(pid, c.b0[idx])
        A_blk = sp.csc_matrix(c.A)[bp]
        A_blk = A_blk[:, np.nonzero(np.asarray(A_blk.sum(axis=0)).ravel() > 0)[0]]
        ref = eng.init_temporal(pid, A_blk, 10, 2, c.deconv)
    finally:
        eng.close()
    K = A_blk.shape[1]
    mex = Mex()
    h = float(mex("create", 0, nout=1)[0, 0])
    try:
        mex("patch", h, 1.0, np.asarray(p, dtype=np.float64), np.asarray(b, dtype=np.float64), c.d1, c.d2, c.T)
        mex("upload", h, 1.0, np.ascontiguousarray(c.Y[:, bp].T), 0)
        with pytest.raises(RuntimeError, match="ring of patch 1 not initialised"):
            mex("init_temporal", h, 1.0, A_blk.astype(np.float64), 10, 2, nout=3)
        mex("ring_init", h, 1.0, c.r, 0)
        mex("set_ring", h, 1.0, sp.csc_matrix(W.T.astype(np.float64)), c.b0[idx].astype(np.float64))
        if c.deconv is None:
            with pytest.raises(RuntimeError, match="with deconvolution only"):
                mex("init_temporal", h, 1.0, A_blk.astype(np.float64), 10, 2, nout=6)
            got = mex("init_temporal", h, 1.0, A_blk.astype(np.float64), 10, 2, nout=3)
            want = (ref[0], ref[1], ref[5])
        else:
            got = mex("init_temporal", h, 1.0, A_blk.astype(np.float64), 10, 2, c.deconv["smin"], c.deconv["max_tau"], nout=6)
            want = (ref[0], ref[1], ref[5], ref[2], ref[3], ref[4])
        assert got[0].shape == (K, c.T) and got[0].dtype == np.float64
        for g, w in zip(got, want):
            assert np.array_equal(g.reshape(w.shape), w.astype(np.float64))
        with pytest.raises(RuntimeError, match="must be sparse"):
            mex("init_temporal", h, 1.0, A_blk.toarray().astype(np.float64), 10, 2, nout=3)
    finally:
        mex("destroy", h)
