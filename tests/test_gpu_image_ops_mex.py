"""The image-operation commands of the MEX gateway -- 'circular_constraints', 'search_dilate', 'trim_spatial' -- through the mock MEX runtime (tests/mex_stub, the
harness of tests/test_gpu_mex_gateway.py) against the ctypes path on the same library: EQUAL results, the gateway only marshals (double -> float, the element
column-major -> row-major, box origins 0-based -> 1-based, bytes -> logical)."""
import os
import sys

import numpy as np
import pytest
import scipy.sparse as sp

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

pytestmark = pytest.mark.gpu


def _assemble(box, off, out, d1, d2, K, dtype):
    """the gateway's boxed result as a d1*d2 x K matrix (what Engine does with the ABI's)"""
    from cnmf_e_amd.engine import Engine
    box = box.T.astype(np.int64).copy(); off = off.ravel().astype(np.int64)
    box[box[:, 2] > 0, :2] -= 1                                          # 1-based origins
    col, pix = Engine._box_cells(box, off, K, d1)
    out = out.ravel()
    nz = np.flatnonzero(out)
    return sp.csc_matrix((out[nz].astype(dtype), (pix[nz], col[nz])), shape=(d1 * d2, K))


@pytest.mark.parametrize("name", ["borders", "big_box"])
def test_the_image_operation_commands_give_the_ctypes_results(name):
    import image_ops_cases as ic
    from test_gpu_mex_gateway import Mex
    from cnmf_e_amd import hostops
    from cnmf_e_amd.engine import Engine
    c = ic.case(name)
    d1, d2, A = c["d1"], c["d2"], c["A"]
    K = A.shape[1]
    se = np.array([[1, 0, 0, 0, 0], [0, 1, 1, 0, 0], [0, 0, 1, 1, 1]], dtype=bool)
    eng = Engine(0)
    try:
        # (the ctypes path without the host's share: the columns the library leaves to the caller are compared as flags)
        circ = eng.circular_constraints(A, d1, d2); dil = eng.search_dilate(A, d1, d2, se, 1, 0.9); trim, small = eng.trim_spatial(A, d1, d2, 0.05, 3, 5)
    finally:
        eng.close()
    mex = Mex()
    h = float(mex("create", 0, nout=1)[0, 0])
    try:
        A64 = A.astype(np.float64)
        box, off, out, hc = mex("circular_constraints", h, A64, d1, d2, nout=4)
        assert box.shape == (4, K) and off.shape == (K + 1, 1) and out.dtype == np.float32 and hc.dtype == np.bool_ and int(hc.sum()) == c["host_columns"]
        dev = np.flatnonzero(~hc.ravel())
        assert np.array_equal(_assemble(box, off, out, d1, d2, K, np.float32)[:, dev].toarray(), circ[:, dev].toarray())
        box, off, out, hc = mex("search_dilate", h, A64, d1, d2, se, 1, 0.9, nout=4)
        assert out.dtype == np.bool_ and int(hc.sum()) == c["host_columns"]
        assert np.array_equal(_assemble(box, off, out, d1, d2, K, bool)[:, dev].toarray(), dil[:, dev].toarray())
        got_d = mex("search_dilate", h, A64, d1, d2, se.astype(np.float64), 1, 0.9, nout=4)[2]                    # a double element
        assert np.array_equal(got_d, out)
        keep, sm, hc = mex("trim_spatial", h, A64, d1, d2, 0.05, 3, 5, nout=3)
        assert keep.dtype == np.bool_ and keep.shape == (A.nnz, 1) and int(hc.sum()) == c["host_columns"]
        got = sp.csc_matrix((A.data * keep.ravel(), A.indices, A.indptr), shape=A.shape)
        assert np.array_equal(got[:, dev].toarray(), trim[:, dev].toarray()) and np.array_equal(sm.ravel()[dev], small[dev])
        with pytest.raises(RuntimeError, match="sz = 4"):
            mex("trim_spatial", h, A64, d1, d2, 0.05, 4, 5, nout=3)
        with pytest.raises(RuntimeError, match="nrgthr"):
            mex("search_dilate", h, A64, d1, d2, se, 1, 1.5, nout=4)
        with pytest.raises(RuntimeError, match="8 inputs"):
            mex("trim_spatial", h, A64, d1, d2, nout=1)
    finally:
        mex("destroy", h)
