"""The merge commands of the MEX gateway -- 'traces_load', 'trace_corr', 'trace_diff_spikes', 'trace_tags', 'merge_apply' -- through the mock MEX runtime
(tests/mex_stub, the harness of tests/test_gpu_mex_gateway.py) against the ctypes path (Engine.*) on the same library: EQUAL arrays, the gateway only marshals
(double -> float, column-major -> the ABI's orders, 1-based rows -> 0-based, float results -> double)."""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

pytestmark = pytest.mark.gpu


def test_the_merge_commands_give_the_ctypes_results():
    import merge_cases as mc
    from test_gpu_mex_gateway import Mex
    from cnmf_e_amd.engine import Engine
    c = mc.case("T403")
    Cm, R, S, kp = c["C"], c["C_raw"], c["S"], c["kernel_pars"]
    K, T = Cm.shape
    groups = [np.array([0, 7]), np.array([1, 8, 9])]
    weights = [np.array([0.25, 0.6]), np.array([0.5, 0.3, 0.2])]
    keep = np.setdiff1d(np.arange(K), [7, 8, 9])
    eng = Engine(0)
    try:
        ref_corr, ref_gram = eng.trace_corr(Cm), eng.trace_corr(R, raw=True)
        ref_sn, ref_diff = eng.trace_diff_spikes(R, want=True)
        ref_dcorr = eng.trace_corr("diff")
        eng.traces_load(Cm, R, S, kp)
        ref_tags = eng.trace_tags()
        ref_apply = eng.merge_apply(groups, weights, keep, None)
        ref_after = eng.trace_corr(ref_apply[0])
    finally:
        eng.close()
    mex = Mex()
    h = float(mex("create", 0, nout=1)[0, 0])
    try:
        d = lambda a: np.asarray(a, dtype=np.float64)
        assert np.array_equal(mex("trace_corr", h, 0, d(Cm), nout=1), ref_corr, equal_nan=True)
        assert np.array_equal(mex("trace_corr", h, 1, R, nout=1), ref_gram)              # a single matrix
        sn, S_ = mex("trace_diff_spikes", h, d(R), nout=2)
        assert np.array_equal(sn.ravel(), ref_sn.astype(np.float64)) and np.array_equal(S_, ref_diff.astype(np.float64))
        assert np.array_equal(mex("trace_corr", h, 0, "diff", K, T, nout=1), ref_dcorr, equal_nan=True)
        with pytest.raises(RuntimeError, match="holds no"):
            mex("trace_tags", h, K, nout=1)                                             # nothing resident yet
        with pytest.raises(RuntimeError, match="unknown source"):
            mex("trace_corr", h, 0, "craww", K, T, nout=1)
        mex("traces_load", h, d(Cm), d(R), d(S), d(kp))
        assert np.array_equal(mex("trace_corr", h, 0, "bound", K, T, nout=1), ref_corr, equal_nan=True)
        assert np.array_equal(mex("trace_corr", h, 1, "craw", K, T, nout=1), ref_gram)
        assert np.array_equal(mex("trace_tags", h, K, nout=1), ref_tags)
        with pytest.raises(RuntimeError, match="frames"):
            mex("merge_apply", h, [0, 2, 5], [1, 8, 2, 9, 10], np.concatenate(weights), keep + 1, T - 1, -5.0, 100.0, nout=5)
        with pytest.raises(RuntimeError, match="must be kept"):
            mex("merge_apply", h, [0, 2, 5], [8, 1, 2, 9, 10], np.concatenate(weights), keep + 1, T, -5.0, 100.0, nout=5)
        out = mex("merge_apply", h, [0, 2, 5], [1, 8, 2, 9, 10], np.concatenate(weights), keep + 1, T, -5.0, 100.0, nout=5)
        for got, ref in zip(out[:3], ref_apply[:3]):
            assert got.shape == (keep.size, T) and np.array_equal(got, ref.astype(np.float64))
        assert np.array_equal(out[3].ravel(), ref_apply[3].astype(np.float64)) and np.array_equal(out[4].ravel(), ref_apply[4].astype(np.float64))
        assert np.array_equal(mex("trace_corr", h, 0, "bound", keep.size, T, nout=1), ref_after, equal_nan=True)
        # the plain delete: no groups
        out = mex("merge_apply", h, np.zeros((0, 0)), np.zeros((0, 0)), np.zeros((0, 0)), [1.0, 3.0], T, -5.0, 100.0, nout=3)
        assert np.array_equal(out[0], ref_apply[0][[0, 2]].astype(np.float64)) and np.array_equal(out[1], ref_apply[1][[0, 2]].astype(np.float64))
    finally:
        mex("destroy", h)
