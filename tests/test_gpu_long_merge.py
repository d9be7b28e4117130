"""cnmfe_trace_tags and cnmfe_trace_diff_spikes beyond the 20 416 frames a trace and its Welch transform share one workgroup's LDS (k_trace_tags_long,
k_trace_diff_spikes_long, csrc/merge.hpp), at the three frame counts of tests/long_cases.py, against float64 NumPy and oasis_oracle.GetSn on the same fp32 values.

GetSn: 2e-4 relative, the bound tests/test_gpu_edges.py::test_get_sn_of_long_recordings asserts of the same estimator at these lengths.  max(C) and the spike
count are exact; std(C_raw - C) is an fp64 sum of fp32 differences in a fixed order: 1e-6 relative.  The thresholded difference trace: S_ equals the oracle's
wherever the oracle's margin |d - 2 sn| / sn exceeds 1.2e-3 (= 2 x the sn bound x 3); at most 0.1 % of a trace's samples may be left out (tests/
test_long_fixtures.py pins the oracle's own share on the CPU) and those are either 0 or the difference.

Observed on the MI355X (20 417 / 40 001 / 74 000; DESIGN.md section 8, "Long recordings"): trace_tags GetSn 4.0e-8 / 4.2e-8 / 4.0e-8, std 1.9e-16;
trace_diff_spikes sn 5.7e-8 / 4.9e-8 / 6.8e-8, no sample left out, S_ equal on every sample.

The methods above the raw calls, at 40 001 frames (long_cases.merge_case: 12 x 10 pixels, seven neurons -- a split pair, a silent row, C_raw == C, three pixels --
whose decision margins tests/test_long_fixtures.py pins): one Sources2D.merge_high_corr and one tag_neurons_parallel + remove_false_positives against
tests/merge_oracle.py.  Groups, newIDs, ids, K and tags equal; the merged column and rows to the tolerances of tests/test_gpu_merge.py (its _check_merge), the
untouched rows bit for bit.  This runs cnmfe_trace_corr, k_merge_rows, k_merge_compact and the long deconvolution inside cnmfe_merge_apply at that length."""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import long_cases as lc
import oasis_oracle as oo

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def eng():
    e = lc.engine()
    yield e
    e.close()


@pytest.mark.parametrize("T", lc.T_LONG)
def test_trace_tags_long(eng, T, observed):
    C, R, S = lc.traces_long(T)
    eng.traces_load(C, R, S)
    q = eng.trace_tags()
    C64, R64 = C.astype(np.float64), R.astype(np.float64)
    sn_ref = np.array([oo.GetSn(r) for r in R64])
    std_ref = np.std(R64 - C64, axis=1, ddof=1)
    e_sn, e_std = float(np.max(np.abs(q[:, 2] - sn_ref) / sn_ref)), float(np.max(np.abs(q[:, 1] - std_ref) / std_ref))
    observed["long_trace_tags_%d" % T] = dict(sn_rel=e_sn, std_rel=e_std)
    print("trace_tags T = %d: GetSn rel %.3e  std rel %.3e" % (T, e_sn, e_std))
    assert np.array_equal(q[:, 0], C64.max(axis=1))
    assert np.array_equal(q[:, 3], (S[:, 1:] > 0).sum(axis=1))
    assert e_std <= 1e-6, e_std
    assert e_sn <= lc.SN_TOL, e_sn


@pytest.mark.parametrize("T", lc.T_LONG)
def test_trace_diff_spikes_long(eng, T, observed):
    R = lc.traces_long(T)[1]
    sn_ref, S_ref, margin = lc.diff_oracle(T)
    sn, S_ = eng.trace_diff_spikes(R, want=True)
    e_sn = float(np.max(np.abs(sn - sn_ref) / sn_ref))
    D = np.c_[np.diff(R.astype(np.float64), axis=1), np.zeros(R.shape[0])]
    firm = margin > lc.DIFF_MARGIN
    left = float((~firm).mean(axis=1).max())
    observed["long_trace_diff_%d" % T] = dict(sn_rel=e_sn, left_out=left, differing=int((S_ != S_ref).sum()))
    print("trace_diff_spikes T = %d: GetSn rel %.3e  left out %.4f %%  samples differing from the oracle %d" % (T, e_sn, 100 * left, int((S_ != S_ref).sum())))
    assert e_sn <= lc.SN_TOL, e_sn
    assert left <= lc.DIFF_LEFT_MAX, left
    assert np.array_equal(S_[firm], S_ref[firm].astype(np.float32))           # (the difference of two fp32 values, rounded to fp32: what the device forms)
    assert np.all((S_[~firm] == 0) | (S_[~firm] == D[~firm].astype(np.float32)))


# ---- the methods at 40 001 frames -----------------------------------------------------------------------------------------------------------------------------
def _merge_sources(eng):
    from cnmf_e_amd.sources2d import PatchedVideo, Sources2D, Options
    c = lc.merge_case()
    video = PatchedVideo(c["d1"], c["d2"], c["T"], [c["d1"], c["d2"]], 3, eng)
    video.upload_from_full(c["video"])
    s = Sources2D(video, Options(ring_radius=3, deconv_flag=True, min_pixel=lc.MERGE_MIN_PIXEL), c["A"], c["C"], c["sn"])
    s.C_raw, s.S = c["C_raw"], c["S"]
    s.P["kernel_pars"] = c["kernel_pars"]
    s.ids = 100 + np.arange(c["A"].shape[1])
    return s, c


def test_merge_high_corr_long(eng):
    import test_gpu_merge as tgm
    s, c = _merge_sources(eng)
    o = lc.merge_oracle_runs()[0]
    before = tgm._before(s)
    merged, newIDs = s.merge_high_corr(merge_thr=lc.MERGE_THR)
    assert [g.tolist() for g in merged] == [g.tolist() for g in o["merged_ROIs"]] == [[0, 6]]
    assert np.array_equal(newIDs, o["newIDs"])
    worst = tgm._check_merge(s, before, o, "long")
    print("merge_high_corr T = %d: %s" % (c["T"], worst))
    assert s.C is eng._bound


def test_tags_and_remove_false_positives_long(eng):
    import test_gpu_merge as tgm
    s, c = _merge_sources(eng)
    _, (ref, _), (ids_ref, o) = lc.merge_oracle_runs()
    tags = s.tag_neurons_parallel()
    assert tags.dtype == np.uint16 and np.array_equal(tags, ref) and np.array_equal(s.tags, ref)
    before = tgm._before(s)
    ids = s.remove_false_positives()
    assert np.array_equal(ids, ids_ref) and ids.tolist() == [2, 3, 4]
    keep = o["keep"]
    assert np.array_equal(s.ids, before["ids"][keep]) and np.array_equal(s.tags, ref[keep])
    assert np.array_equal(np.asarray(s.C), before["C"][keep]) and np.array_equal(np.asarray(s.C_raw), before["C_raw"][keep]) and np.array_equal(np.asarray(s.S), before["S"][keep])
    assert np.array_equal(np.asarray(s.P["kernel_pars"]), before["kp"][keep]) and np.array_equal(s.A.toarray(), before["A"][:, keep].toarray())
    assert s.C is eng._bound
