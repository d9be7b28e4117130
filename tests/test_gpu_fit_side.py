"""The ring fit's set-up after it moved (bg.hip): the pair / need / work / tile tables kept with the patch instead of computed and uploaded every fit, sum(A, 2) and
slot_of built on the device instead of uploaded, and -- option fit_side -- everything between the window projection and k_win_fix queued on a second stream.
None of it may change a value: the same kernels run on the same numbers.

* tests/golden/fit_setup_parent.npz holds what the runs of tests/fit_side_cases.py gave on the commit before the move (scripts/make_fit_setup_golden.py, on the
  MI355X with that commit's library; never written by a later build): sampled rows of W, b0 and the info of every fit, A and C after the full iterations.
* every case runs under fit_side = 0 (one stream, the old order), 1 (the set-up beside the projection) and 2 (the same streams, joined in front of the
  projection); each must equal the golden, and so each other, under np.array_equal.
* the profiled cases also show that the later fits are steady-state fits (the window projection ran, no table build) and that the device-side builders ran."""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(ROOT, "oracle"))

import fit_side_cases as fc

GOLDEN = os.path.join(HERE, "golden", "fit_setup_parent.npz")
_RUNS = {}                                                   # (case, fit_side) -> arrays of the runs so far


@pytest.fixture(scope="module")
def golden():
    with np.load(GOLDEN) as z:
        return {k: z[k] for k in z.files}


def _of_case(golden, name):
    return {k.split("/", 1)[1]: v for k, v in golden.items() if k.startswith(name + "/")}


def test_golden_file_covers_every_case(golden):
    assert os.path.getsize(GOLDEN) < 400 * 1024
    for name in fc.CASES:
        ref = _of_case(golden, name)
        assert any(k.endswith("_W") for k in ref) and any(k.endswith("_b0") for k in ref) and any(k.endswith("_info") for k in ref), name
        if name in fc.SRC:
            assert {"A_data", "A_indices", "A_indptr", "C"} <= set(ref), name


def _same(name, what, a, b):
    assert a.keys() == b.keys(), (name, what, sorted(set(a) ^ set(b)))
    for k in a:
        assert a[k].shape == b[k].shape and a[k].dtype == b[k].dtype, (name, what, k, a[k].shape, b[k].shape)
        assert np.array_equal(a[k], b[k]), (name, what, k, int((a[k] != b[k]).sum()), a[k].size)


@pytest.mark.gpu
@pytest.mark.parametrize("fit_side", [0, 1, 2])
@pytest.mark.parametrize("name", fc.CASES)
def test_fit_setup_equals_the_parent(golden, name, fit_side):
    got, extra = fc.run_case(name, fit_side)
    _same(name, "fit_side %d against the parent" % fit_side, _of_case(golden, name), got)
    for (n, m), other in _RUNS.items():
        if n == name:
            _same(name, "fit_side %d against %d" % (fit_side, m), other, got)
    _RUNS[(name, fit_side)] = got
    infos = {k: v for k, v in got.items() if k.endswith("_info")}
    firsts = [k for k, v in infos.items() if v[0]]
    assert firsts and all(k.startswith(("it0_", "fit0_", "e0_fit0", "e1_fit0")) for k in firsts), firsts      # only a patch's first fit is a first run
    if name in ("i_r5", "ii_fp32"):
        assert len(extra) == 3
        assert any(k.startswith("bg_gram_") for k in extra[0]) and "bg_slot_table" in extra[0]               # the first fit builds the video's table
        for ks in extra[1:]:                                                                                 # fits 2 and 3: the window projection, no table build
            assert "bg_win_proj" in ks and "bg_win_fix" in ks and not any(k.startswith("bg_gram_") for k in ks), sorted(ks)
            assert {"bg_asum", "bg_slot_table", "bg_trace_subsum", "bg_active", "bg_b0"} <= ks, sorted(ks)
            assert ("bg_trace_gram" in ks) == (name == "i_r5"), sorted(ks)
    if name == "v_stride":
        import cnmfe_oracle as orc
        assert [int(got["fit%d_info" % k][1]) for k in range(5)] == list(fc.STRIDES)
        assert [orc.ring_frame_stride(W, fc.STRIDE_T) for W in extra] == list(fc.STRIDES)
        assert [int(got["fit%d_info" % k][3]) for k in range(1, 5)] == list(fc.STRIDE_M[1:])
