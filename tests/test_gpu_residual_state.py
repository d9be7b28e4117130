"""The residual's bookkeeping after it moved into one struct and one plan (common.hpp: ResidualState, FootTerm; residual_plan.hpp): no kernel, launch or option
changed, so every sequence of tests/residual_state_cases.py must give the bits AND the launches of the commit before the move.

* tests/golden/residual_state_parent.npz holds what the sequences gave on that commit (scripts/make_residual_state_golden.py, on the MI355X with that commit's
  library; never written by a later build).
* each case runs on a fresh engine; every recorded array must equal the golden under np.array_equal, and so must the call counts of the residual's kernels
  (the same plan means the same launches).  The two error messages a sequence ends on are recorded arrays like the rest."""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import residual_state_cases as rc

GOLDEN = os.path.join(HERE, "golden", "residual_state_parent.npz")
FIT_SETUP_GOLDEN = os.path.join(HERE, "golden", "fit_setup_parent.npz")


@pytest.fixture(scope="module")
def golden():
    with np.load(GOLDEN) as z:
        return {k: z[k] for k in z.files}


def _of_case(golden, name):
    return {k.split("/", 1)[1]: v for k, v in golden.items() if k.startswith(name + "/")}


def test_golden_file_covers_every_case(golden):
    assert os.path.getsize(GOLDEN) <= os.path.getsize(FIT_SETUP_GOLDEN)
    assert str(golden["commit"]) and len(rc.CASES) == 16
    for name, (shape, _) in rc.CASES.items():
        ref = _of_case(golden, name)
        have = {k[:-len(suffix)] if k.endswith(suffix) else k for k in ref for suffix in ("_sample", "_sums", "_rows")}        # (large arrays: sample / rows + sums)
        want = {"01_b0", "04_A_indptr", "04_A_indices", "04_A_data", "06_C", "06_Craw", "06_aa", "07_sn", "08_ysig", "10_ysig", "14_error", "kernels", "calls"}
        want |= {"09_rss_error"} if shape == "ssub" else {"11_rss", "12_bg"}
        assert want <= have, (name, sorted(want - have))
        assert all(k + "_sums" in ref for k in ("08_ysig", "10_ysig", "01_b0", "07_sn")), name
        assert str(ref["14_error"]) == rc.NOT_RUN


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(rc.CASES))
def test_residual_sequences_equal_the_parent(golden, name):
    ref, got = _of_case(golden, name), rc.run_case(name)
    assert dict(zip(got["kernels"].tolist(), got["calls"].tolist())) == dict(zip(ref["kernels"].tolist(), ref["calls"].tolist()))
    assert ref.keys() == got.keys(), (name, sorted(set(ref) ^ set(got)))
    for k in ref:
        assert ref[k].shape == got[k].shape and ref[k].dtype == got[k].dtype, (name, k, ref[k].shape, got[k].shape)
        assert np.array_equal(ref[k], got[k]), (name, k, int((ref[k] != got[k]).sum()), ref[k].size)
