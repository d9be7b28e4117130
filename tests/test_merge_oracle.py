"""The merge fixtures and the host half of the merges, on the CPU: the decision margins of every fixture (conditions, not measurements: no accuracy the device
can plausibly have may flip a decision), the Gram-space form of a group's alternation against the literal one, the connected components against a brute-force
labelling, and the flat row."""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import merge_cases as mc
import merge_oracle as mo
from cnmf_e_amd import hostops

EXPECT = {   # the groups the fixtures were built for (merge_cases.py)
    "high_corr": [[0, 7], [1, 8, 9]], "high_corr_scalar": [[0, 7], [1, 8, 9]], "high_corr_decay": None,
    "dist_corr": [[0, 7], [1, 8, 9]], "dist_corr_decay": None, "close": [[0, 7], [1, 8, 9], [2, 10]],
}


@pytest.mark.parametrize("name", sorted(mc.CASES))
@pytest.mark.parametrize("call", sorted(mc.CALLS))
def test_decision_margins(name, call):
    out = mc.oracle_call(name, call)
    mg = out["margins"]
    print(name, call, dict(mg), [g.tolist() for g in out["merged_ROIs"]])
    for key in ("A_overlap", "C_corr", "S_corr", "dist"):
        if key in mg:
            assert mg[key] >= mc.MARGIN, (key, mg[key])
    if EXPECT[call] is not None:
        assert [g.tolist() for g in out["merged_ROIs"]] == EXPECT[call]
    else:
        assert len(out["merged_ROIs"]) >= 1                                     # (the decay bound decides on the host from the same float32 kernel_pars on both sides)
    assert all(3 not in g for g in out["merged_ROIs"])                          # the flat row never merges
    assert out["C"].shape[0] == 12 - sum(len(g) - 1 for g in out["merged_ROIs"])


@pytest.mark.parametrize("name", sorted(mc.CASES))
def test_margins_without_S_and_tags(name):
    c = mc.case(name)
    out = mo.merge_high_corr(c["A"], c["C_raw"], c["C_raw"], None, None, [0.1, 0.5, 0.3])      # deconv_flag = false: C is C_raw, there is no S
    mg = out["margins"]
    print(name, dict(mg), [g.tolist() for g in out["merged_ROIs"]])
    assert mg["diff_cut"] >= mc.MARGIN_CUT and mg["C_corr"] >= mc.MARGIN and mg["S_corr"] >= mc.MARGIN and mg["A_overlap"] >= mc.MARGIN
    assert all(3 not in g for g in out["merged_ROIs"])
    tags, tm = mo.tag_neurons(c["A"], c["C"], c["C_raw"], c["S"], mc.MIN_PIXEL)
    print(name, tags.tolist(), dict(tm))
    assert tm["noise_ratio"] >= mc.MARGIN_TAG and tm["pnr"] >= mc.MARGIN_TAG
    assert tags[11] & 1 and tags[4] & 2 and tags[3] & 2 and tags[5] & 4
    assert tags[6] == 0 and not (tags[np.array([0, 1, 2, 6, 7, 8, 9, 10])] & 1).any()


@pytest.mark.parametrize("name", sorted(mc.CASES))
def test_gram_space_iteration_equals_the_literal_one(name):
    """fp64 algebra: ai = A(:, IDs) g and ci = w' C_raw(IDs, :) of hostops.merge_iterate against the alternation on `data`, 1e-10 relative"""
    c = mc.case(name)
    out = mc.oracle_call(name, "close")
    A = np.asarray(c["A"].todense(), dtype=np.float64); R = c["C_raw"].astype(np.float64)
    for IDs, (active, ai_ref), ci_ref in zip(out["merged_ROIs"], out["ai"], out["ci"]):
        g, w = hostops.merge_iterate(R[IDs] @ R[IDs].T, A[:, IDs].T @ A[:, IDs])
        ai = A[np.ix_(active, IDs)] @ g
        ci = w @ R[IDs]
        assert np.linalg.norm(ai - ai_ref) <= 1e-10 * np.linalg.norm(ai_ref)
        assert np.linalg.norm(ci - ci_ref) <= 1e-10 * np.linalg.norm(ci_ref)


def test_connected_components_match_brute_force():
    rng = np.random.default_rng(3)
    for K, p in ((0, 0.0), (1, 0.0), (7, 0.2), (16, 0.08), (33, 0.03), (33, 0.0)):
        flag = rng.random((K, K)) < p
        flag = flag | flag.T
        got = [g.tolist() for g in hostops.merge_groups(flag)]
        assert got == [g.tolist() for g in mo.groups_of(flag)], (K, p)
    chain = np.zeros((5, 5), dtype=bool); chain[0, 2] = chain[2, 0] = chain[2, 4] = chain[4, 2] = True
    assert [g.tolist() for g in hostops.merge_groups(chain)] == [[0, 2, 4]]


def test_host_helpers_equal_the_oracle():
    c = mc.case("T403")
    yy, xx = hostops.neuron_centers(c["A"], c["d1"], c["d2"], "max")
    yo, xo = mo.centers(c["A"], c["d1"], c["d2"], "max")
    assert np.array_equal(yy, yo) and np.array_equal(xx, xo)
    yy, xx = hostops.neuron_centers(c["A"], c["d1"], c["d2"], "mean")
    yo, xo = mo.centers(c["A"], c["d1"], c["d2"], "mean")
    assert np.allclose(yy, yo, rtol=0, atol=1e-9) and np.allclose(xx, xo, rtol=0, atol=1e-9)     # (float32 footprints summed in another order)
    Ad = np.asarray(c["A"].todense(), dtype=np.float64)
    temp = Ad / np.sqrt((Ad ** 2).sum(axis=0))
    assert np.allclose(hostops.footprint_overlap(c["A"]), temp.T @ temp, rtol=0, atol=1e-12)
    assert np.array_equal(hostops.decay_times(c["kernel_pars"]), mo.ar2exp1(c["kernel_pars"]))


def test_flat_row_correlates_with_nothing():
    c = mc.case("T400")
    r = mo.corr_rows(c["C"])
    assert np.isnan(r[3]).all() and np.isnan(r[:, 3]).all() and np.isfinite(np.delete(np.delete(r, 3, 0), 3, 1)).all()
    assert not (r[3] >= -1.0).any()                                             # NaN fails every >=
