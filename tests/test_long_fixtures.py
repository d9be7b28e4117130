"""CPU: the fixtures of the long-recording GPU tests (tests/long_cases.py) are what those tests assume -- the shares they leave out and the decision margins of
the oracle's runs are recomputed here from the oracle alone, so the caps and the forced seeds are pinned without a GPU."""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import greedy_cases as gc
import long_cases as lc


@pytest.mark.parametrize("T,share", [(20417, 0.025), (40001, 0.0), (74000, 0.0)])
def test_quantised_seed_video_leaves_few_pixels_out(T, share):
    """the quantised video without filter: the oracle's fragile pixels and their neighbours are 2.5 %, 0 %, 0 % of the 20 x 18 block -- under the 10 % cap"""
    Cn, PNR, robust = lc.seed_oracle_q(T)
    left = float((~robust).mean())
    assert left <= lc.SEED_LEFT_MAX and abs(left - share) < 1e-9, left
    assert np.all(np.isfinite(Cn)) and np.all(np.abs(Cn) <= 1.0) and np.all(PNR > 0)


@pytest.mark.parametrize("T", lc.T_LONG)
def test_difference_traces_leave_few_samples_out(T):
    sn, S_, margin = lc.diff_oracle(T)
    assert np.all(sn > 0) and S_.any()
    assert float((margin <= lc.DIFF_MARGIN).mean(axis=1).max()) <= lc.DIFF_LEFT_MAX


def _check_forced(T):
    fr = lc.peel_oracle(T, forced=True)
    assert [tuple(int(x) for x in rc) for rc in fr["center"]] == lc.PEEL_CENTRES[T]
    assert fr["margins"]["corr"] >= gc.MARGIN_MIN["corr"], fr["margins"]["corr"]
    steps = fr["blocks"][(0, 0)]["steps"]
    assert [s["kind"] for s in steps] == ["extract", "apply"] * len(lc.PEEL_CENTRES[T])
    for s in steps:
        if s["kind"] == "apply":
            assert (s["pnr"] != 0).mean() >= 0.5                      # the PNR box the GPU test compares: at least half of it non-zero in the oracle alone
        else:
            assert s["ai"] is not None and all(np.isfinite(v) and v > 0 for v in s["stats"].values())


def test_peel_fixture_20417():
    """the automatic search accepts the pinned centres with the corr margins cleared, a centre lies within 2 pixels of each true one, and the forced run of
    those centres accepts them again; the C row of that centre correlates above 0.9 with the true trace (0.994 and 0.989)."""
    T = 20417
    auto = lc.peel_oracle(T, forced=False)
    assert [tuple(int(x) for x in rc) for rc in auto["center"]] == lc.PEEL_CENTRES[T]
    assert auto["margins"]["corr"] >= gc.MARGIN_MIN["corr"], auto["margins"]["corr"]
    f, _ = lc.peel_video(T)
    for k in range(f.K):
        tr = np.unravel_index(int(np.argmax(f.A_true[:, k].toarray().ravel())), lc.PEEL["dims"], order="F")
        dist = [max(abs(r - 1 - tr[0]), abs(c - 1 - tr[1])) for r, c in lc.PEEL_CENTRES[T]]
        j = int(np.argmin(dist))
        assert dist[j] <= 2
        assert np.corrcoef(auto["C"][j], f.C_true[k])[0, 1] > 0.9
    _check_forced(T)


def test_peel_fixture_74000():
    _check_forced(74000)


def test_merge_fixture_40001():
    """the 12 x 10 x 40 001 merge fixture: every K x K decision of merge_high_corr clears the margin tests/test_merge_oracle.py asks of the short fixtures, the tag
    ratios theirs; the split pair merges and nothing else, the silent row, the C_raw == C row and the three-pixel neuron are the ones deleted"""
    import merge_cases as mc
    m, (tags, tm), (ids, kept) = lc.merge_oracle_runs()
    mg = m["margins"]
    assert mg["A_overlap"] >= mc.MARGIN and mg["C_corr"] >= mc.MARGIN and mg["S_corr"] >= mc.MARGIN, dict(mg)
    assert [g.tolist() for g in m["merged_ROIs"]] == [[0, 6]] and m["newIDs"].tolist() == [0]
    assert tm["noise_ratio"] >= mc.MARGIN_TAG and tm["pnr"] >= mc.MARGIN_TAG, dict(tm)
    assert tags.tolist() == [0, 0, 2, 4, 1, 0, 0] and ids.tolist() == [2, 3, 4]
    c = lc.merge_case()
    assert c["video"].shape == (lc.MERGE_T, 120) and c["C"].shape == (7, lc.MERGE_T)
