"""Merging and tagging on the engine against the literal float64 oracle (tests/merge_oracle.py) on the fixtures of tests/merge_cases.py, whose decision margins
tests/test_merge_oracle.py pins on the CPU: the discrete results (groups, newIDs, ids, K, tags) are equal, the merged column and raw trace agree to the rounding of
their float32 storage, the merged row's deconvolution to the tolerances of tests/test_gpu_parity.py::test_deconv_temporal_parity, untouched rows bit for bit."""
import os
import sys

import numpy as np
import pytest
import scipy.sparse as sp

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, os.path.join(ROOT, "oracle"))
sys.path.insert(0, HERE)
pytestmark = pytest.mark.gpu

import merge_cases as mc
import merge_oracle as mo
from parity_util import rel

# Observed on the MI355X (profiles/merge/parity_observed.json, merged_max: the largest value over both fixtures, all calls and the S-less branch): merged A column
# 2.9e-8, merged C_raw row 2.8e-8 of the literal float64 result -- the rounding of their float32 storage.  The asserts are ten times that (the rule of
# tests/test_gpu_zconfigs.py:73), far inside the 3e-6 / 5e-6 of tests/test_gpu_kchange.py.
TOL_A, TOL_CRAW = 2.9e-7, 2.8e-7
# the merged row's deconvolution: exactly tests/test_gpu_parity.py::test_deconv_temporal_parity
TOL_C, TOL_PARS, TOL_SN = 5e-6, 2e-6, 5e-6
KS = (0, 1, 15, 16, 17, 33)


@pytest.fixture(scope="module")
def eng():
    from cnmf_e_amd.engine import Engine
    e = Engine(0)
    yield e
    e.close()


def _sources(eng, name, deconv=True):
    from cnmf_e_amd.sources2d import PatchedVideo, Sources2D, Options
    c = mc.case(name)
    video = PatchedVideo(c["d1"], c["d2"], c["T"], [c["d1"], c["d2"]], 6, eng)
    video.upload_from_full(c["video"])
    if deconv:
        s = Sources2D(video, Options(ring_radius=6, deconv_flag=True, min_pixel=mc.MIN_PIXEL), c["A"], c["C"], c["sn"])
        s.C_raw, s.S = c["C_raw"], c["S"]
        s.P["kernel_pars"] = c["kernel_pars"]
    else:                                                   # deconv_flag = false: C_raw is C, there is no S and no kernel_pars
        s = Sources2D(video, Options(ring_radius=6, deconv_flag=False, min_pixel=mc.MIN_PIXEL), c["A"], c["C_raw"], c["sn"])
        s.C_raw = s.C
    s.ids = 100 + np.arange(12)
    return s, c


def _check_merge(s, before, o, tag):
    """s: the Sources2D after the merge, before: dict of its arrays before, o: the oracle's result"""
    keep = o["keep"]
    assert s.A.shape[1] == len(keep) == np.asarray(s.C).shape[0] == np.asarray(s.C_raw).shape[0]
    assert np.array_equal(s.ids, before["ids"][keep])
    merged_new = set(o["newIDs"].tolist())
    A = s.A.toarray().astype(np.float64)
    worst = {"A": 0.0, "C_raw": 0.0, "C": 0.0, "pars": 0.0}
    for j, k in enumerate(keep):
        if j in merged_new:
            eA, eR, eC = rel(A[:, j], o["A"][:, j]), rel(np.asarray(s.C_raw)[j], o["C_raw"][j]), rel(np.asarray(s.C)[j], o["C"][j])
            eP = abs(float(np.asarray(s.P["kernel_pars"])[j]) - o["kernel_pars"][j])
            print("MERGE_OBSERVED", tag, "row", j, "A", eA, "C_raw", eR, "C", eC, "pars", eP)
            worst = {"A": max(worst["A"], eA), "C_raw": max(worst["C_raw"], eR), "C": max(worst["C"], eC), "pars": max(worst["pars"], eP)}
            if o["S"] is not None:
                eg, er = np.nonzero(np.asarray(s.S)[j] > 0)[0], np.nonzero(o["S"][j] > 0)[0]
                assert abs(len(eg) - len(er)) <= 1, (tag, j, len(eg), len(er))
        else:                                               # untouched rows and columns: bit for bit
            assert np.array_equal(s.A[:, [j]].toarray(), before["A"][:, [int(k)]].toarray()), (tag, j)
            assert np.array_equal(np.asarray(s.C)[j], before["C"][k]) and np.array_equal(np.asarray(s.C_raw)[j], before["C_raw"][k]), (tag, j)
            if before["S"] is not None:
                assert np.array_equal(np.asarray(s.S)[j], before["S"][k]), (tag, j)
            if before["kp"] is not None:
                assert np.asarray(s.P["kernel_pars"])[j] == before["kp"][k]
    assert worst["A"] <= TOL_A and worst["C_raw"] <= TOL_CRAW, (tag, worst)
    assert worst["C"] <= TOL_C and worst["pars"] <= TOL_PARS, (tag, worst)
    return worst


def _before(s):
    S = getattr(s, "S", None)
    kp = s.P.get("kernel_pars")
    return dict(A=s.A.copy(), C=np.array(s.C), C_raw=np.array(s.C_raw), S=None if S is None else np.array(S), kp=None if kp is None else np.array(kp), ids=s.ids.copy())


# ---- correlation and Gram -------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("T", [400, 403])
@pytest.mark.parametrize("K", KS)
def test_trace_corr_and_gram(eng, K, T):
    """cnmfe_trace_corr against np.corrcoef in float64 of the same fp32 values, the raw Gram against the float64 product: absolute error <= 1e-10 (fp64 accumulation
    of T <= 403 terms of unit scale, about 5e-14, times a thousand), the NaN pattern equal, two calls bit-identical"""
    X = mc.traces(K, T)
    X64 = X.astype(np.float64)
    got, got2 = eng.trace_corr(X), eng.trace_corr(X)
    raw, raw2 = eng.trace_corr(X, raw=True), eng.trace_corr(X, raw=True)
    assert got.shape == (K, K) and got.tobytes() == got2.tobytes() and raw.tobytes() == raw2.tobytes()
    if K == 0:
        return
    with np.errstate(divide="ignore", invalid="ignore"):
        ref = np.corrcoef(X64).reshape(K, K)
    assert np.array_equal(np.isnan(got), np.isnan(ref))
    if K >= 15:
        assert np.isnan(got[K - 2]).all() and np.isnan(got[:, K - 2]).all() and np.isnan(got).sum() == 2 * K - 1
    ok = ~np.isnan(ref)
    e_c, e_g = np.abs(got[ok] - ref[ok]).max(), np.abs(raw - X64 @ X64.T).max()
    print("CORR_OBSERVED K", K, "T", T, "corr", e_c, "gram", e_g)
    assert e_c <= 1e-10 and e_g <= 1e-10, (e_c, e_g)
    assert np.array_equal(raw, raw.T) and np.array_equal(got[ok], got.T[ok])


def test_trace_corr_sources_agree(eng):
    """the bound matrix, the residents and a host matrix are the same kernel on the same values: bit-identical; column-major input too"""
    import ctypes as C
    from cnmf_e_amd import _lib as L
    X, Y, Z = mc.traces(17, 403), mc.traces(17, 403, seed=6), mc.traces(17, 403, seed=7)
    ref = [eng.trace_corr(M) for M in (X, Y, Z)]
    eng.traces_load(X, Y, Z)
    n0 = eng.counter("merge_trace_uploads")
    for M, r in zip((X, Y, Z), ref):
        assert eng.trace_corr(M).tobytes() == r.tobytes()
    assert eng.counter("merge_trace_uploads") == n0
    Xf = np.asfortranarray(X)
    out = np.empty((17, 17))
    L.check(L.lib.cnmfe_trace_corr(eng._ctx, 17, 403, Xf.ctypes.data_as(L.f32p), L.COLMAJOR, 0, out.ctypes.data_as(L.f64p)))
    assert out.tobytes() == ref[0].tobytes()
    assert eng.counter("merge_trace_uploads") == n0 + 1
    eng.bind_traces(None)


# ---- the three merges through Sources2D ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(mc.CASES))
@pytest.mark.parametrize("call", sorted(mc.CALLS))
def test_merge_methods(eng, name, call):
    s, c = _sources(eng, name)
    o = mc.oracle_call(name, call)
    before = _before(s)
    meth, kw = mc.CALLS[call]
    merged, newIDs = getattr(s, meth)(**kw)
    assert [g.tolist() for g in merged] == [g.tolist() for g in o["merged_ROIs"]]
    assert np.array_equal(newIDs, o["newIDs"])
    _check_merge(s, before, o, "%s/%s" % (name, call))
    assert s.C is eng._bound and s.A_prev.shape[1] == 12 and s.C_prev.shape[0] == 12          # A_prev, C_prev stay (the reference leaves them too)
    b0 = s.b0_new
    ref = (s.ymean_full() - np.asarray(s.A @ np.asarray(s.C).mean(axis=1, dtype=np.float64)).ravel()).reshape(c["d1"], c["d2"], order="F")
    assert np.allclose(b0, ref, rtol=0, atol=1e-9 * max(1.0, np.abs(ref).max()))                  # b0_new follows the merge (update_spatial_parallel.m:349's expression)


@pytest.mark.parametrize("name", sorted(mc.CASES))
def test_merge_high_corr_without_S(eng, name):
    """deconv_flag = false, no S: the spike trains are the thresholded differences of C_raw, taken on the device (merge_high_corr.m:57-66); S stays absent"""
    s, c = _sources(eng, name, deconv=False)
    R = c["C_raw"]
    sn, S_ = eng.trace_diff_spikes(R, want=True)
    S_ref = mo.diff_spikes(R)
    import oasis_oracle as oo
    sn_ref = np.array([oo.GetSn(np.r_[np.diff(r.astype(np.float64)), 0.0]) for r in R])
    assert np.allclose(sn, sn_ref, rtol=TOL_SN)
    assert np.array_equal(S_ == 0, S_ref == 0) and np.abs(S_ - S_ref).max() <= 1e-6 * np.abs(S_ref).max()
    o = mo.merge_high_corr(c["A"], R, R, None, None, [0.1, 0.5, 0.3])
    before = _before(s)
    merged, newIDs = s.merge_high_corr(merge_thr=[0.1, 0.5, 0.3])
    assert [g.tolist() for g in merged] == [g.tolist() for g in o["merged_ROIs"]] and len(merged) >= 1
    assert np.array_equal(newIDs, o["newIDs"])
    _check_merge(s, before, o, "%s/no S" % name)
    assert getattr(s, "S", None) is None                    # absent stays absent


def test_nothing_to_merge_touches_nothing(eng):
    s, c = _sources(eng, "T400")
    s._bind_C()
    A0, C0, R0, S0, bound0 = s.A, s.C, s.C_raw, s.S, eng._bound
    Cv = np.array(C0)
    merged, newIDs = s.merge_high_corr(merge_thr=[0.1, 2.0, 0.3])           # no correlation reaches 2
    assert merged == [] and len(newIDs) == 0
    merged, newIDs = s.merge_neurons_dist_corr(merge_thr=2.0, dmin=mc.DMIN)
    assert merged == [] and len(newIDs) == 0
    assert s.A is A0 and s.C is C0 and s.C_raw is R0 and s.S is S0 and eng._bound is bound0 and bound0 is C0
    assert np.array_equal(np.asarray(s.C), Cv)
    # the device's bound matrix is still that C: a correlation of it needs no upload and equals the host path's
    n0 = eng.counter("merge_trace_uploads")
    r = eng.trace_corr(s.C)
    assert eng.counter("merge_trace_uploads") == n0
    assert r.tobytes() == eng.trace_corr(Cv).tobytes()


def test_unbuilt_options_raise(eng):
    s, _ = _sources(eng, "T400")
    with pytest.raises(NotImplementedError):
        s.merge_high_corr(show_merge=True)
    s.options.deconv_options = dict(s.options.deconv_options, method="thresholded")
    for m in ("merge_high_corr", "merge_neurons_dist_corr", "merge_close_neighbors"):
        with pytest.raises(NotImplementedError):
            getattr(s, m)()


# ---- tags and deletion -----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(mc.CASES))
def test_tags_and_remove_false_positives(eng, name):
    s, c = _sources(eng, name)
    ref, _ = mo.tag_neurons(c["A"], c["C"], c["C_raw"], c["S"], mc.MIN_PIXEL)
    tags = s.tag_neurons_parallel()
    assert tags.dtype == np.uint16 and np.array_equal(tags, ref) and np.array_equal(s.tags, ref)
    q = eng.trace_tags()
    import oasis_oracle as oo
    C64, R64 = c["C"].astype(np.float64), c["C_raw"].astype(np.float64)
    assert np.array_equal(q[:, 0], C64.max(axis=1)) and np.array_equal(q[:, 3], (c["S"][:, 1:] > 0).sum(axis=1))
    assert np.allclose(q[:, 1], np.std(R64 - C64, axis=1, ddof=1), rtol=1e-12, atol=0) and q[5, 1] == 0.0
    assert np.allclose(q[:, 2], [oo.GetSn(r) for r in R64], rtol=TOL_SN)
    before = _before(s)
    ids = s.remove_false_positives()
    ids_ref, o = mo.remove_false_positives(c["A"], c["C"], c["C_raw"], c["S"], c["kernel_pars"], mc.MIN_PIXEL)
    assert np.array_equal(ids, ids_ref) and ids.tolist() == [3, 4, 5, 11]
    keep = o["keep"]
    assert np.array_equal(s.ids, before["ids"][keep]) and np.array_equal(s.tags, ref[keep])
    assert np.array_equal(np.asarray(s.C), before["C"][keep]) and np.array_equal(np.asarray(s.C_raw), before["C_raw"][keep]) and np.array_equal(np.asarray(s.S), before["S"][keep])
    assert np.array_equal(np.asarray(s.P["kernel_pars"]), before["kp"][keep]) and np.array_equal(s.A.toarray(), before["A"][:, keep].toarray())
    assert s.C is eng._bound
    assert eng.trace_corr(s.C).tobytes() == eng.trace_corr(before["C"][keep]).tobytes()       # the compacted device matrix is that C


# ---- traffic and state after a merge ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pdims", [None, [36, 36]])
def test_state_after_merge_and_traffic(eng, pdims):
    """tests/test_gpu_kchange.py's pattern with the real methods: one iteration on both sides, merge_neurons_dist_corr + merge_high_corr + remove_false_positives on
    both sides (the oracle's from its own float64 state; the decisions are asserted to be clear of their thresholds and equal), then a spatial -> temporal round
    without a background update and a full round, at that file's tolerances.  On the way: after update_temporal_parallel with deconvolution the merge and tag calls
    take no K x T matrix from the host."""
    import cnmfe_oracle as orc
    from cnmf_e_amd import synth
    from cnmf_e_amd.sources2d import PatchedVideo, Sources2D, Options
    d1, d2, T, K, r = 72, 72, 600, 12, 15
    f = synth.make_factors(d1, d2, T, K, 17, gSig=2.0, gSiz=9, min_sep=6)
    # neuron 1 becomes a second, dimmer view of neuron 0: two pixel rows lower, neuron 0's activity plus half of its own
    A_true = sp.lil_matrix(f.A_true); A_init = sp.lil_matrix(f.A_init)
    A_true[:, 1] = sp.csc_matrix(mc._shift(np.asarray(f.A_true[:, 0].todense()).ravel(), d1, d2, 2, 0)[:, None] * 0.7)
    A_init[:, 1] = sp.csc_matrix(mc._shift(np.asarray(f.A_init[:, 0].todense()).ravel(), d1, d2, 2, 0)[:, None] * 0.7)
    f.A_true, f.A_init = sp.csc_matrix(A_true), sp.csc_matrix(A_init)
    f.C_true[1] = f.C_true[0] + 0.5 * f.C_true[1]; f.C_init[1] = f.C_init[0] + 0.5 * f.C_init[1]     # (some activity of its own: the two stay separable for the updates)
    Y = synth.make_video(f, np.float32)
    video = PatchedVideo(d1, d2, T, pdims or [d1, d2], r, eng)
    video.upload_from_full(Y)
    s = Sources2D(video, Options(ring_radius=r, spatial_algorithm="hals", maxIter=3, deconv_flag=True, min_pixel=5), f.A_init, f.C_init, f.sn)
    o = orc.OracleSources2D(Y.T.reshape(d1, d2, T, order="F"), d1, d2, T, pdims or [d1, d2], r, f.A_init.astype(np.float32), f.C_init, f.sn,
                            spatial_algorithm="hals", maxIter=3, deconv_options={})
    def both(name):
        getattr(s, name)(); getattr(o, name)()
    def check(tag, tolA=3e-6, tolC=5e-6):
        eA, eC, eR = rel(s.A.toarray(), o.A.toarray()), rel(np.asarray(s.C), o.C), rel(np.asarray(s.C_raw), o.C_raw)
        print("STATE_OBSERVED", pdims, tag, eA, eC, eR)
        assert s.A.shape == o.A.shape and np.asarray(s.C).shape == o.C.shape
        assert eA <= tolA and eC <= tolC and eR <= tolC, (tag, eA, eC, eR)
    for m in ("update_background_parallel", "update_spatial_parallel", "update_temporal_parallel"):
        both(m)
    check("iteration 1")
    n0 = eng.counter("merge_trace_uploads")
    # ---- the demo's calls between the updates (demo_large_data_1p.m:205-207), on both sides ----
    def oracle_set(res):
        o.A, o.C, o.C_raw, o.S, o.kernel_pars = sp.csc_matrix(res["A"]), res["C"], res["C_raw"], res["S"], res["kernel_pars"]
    g_all = []
    res = mo.merge_neurons_dist_corr(o.A, o.C, o.C_raw, o.S, o.kernel_pars, d1, d2, 0.5, mc.DMIN)
    assert res["margins"]["C_corr"] >= mc.MARGIN
    merged, _ = s.merge_neurons_dist_corr(merge_thr=0.5, dmin=mc.DMIN)
    assert [g.tolist() for g in merged] == [g.tolist() for g in res["merged_ROIs"]]
    g_all += merged; oracle_set(res)
    res = mo.merge_high_corr(o.A, o.C, o.C_raw, o.S, o.kernel_pars, [0.1, 0.5, 0.3])
    assert min(res["margins"][k] for k in ("A_overlap", "C_corr", "S_corr")) >= mc.MARGIN
    merged, _ = s.merge_high_corr(merge_thr=[0.1, 0.5, 0.3])
    assert [g.tolist() for g in merged] == [g.tolist() for g in res["merged_ROIs"]]
    g_all += merged; oracle_set(res)
    tags_ref, tm = mo.tag_neurons(o.A, o.C, o.C_raw, o.S, 5)
    assert tm["noise_ratio"] >= mc.MARGIN_TAG and tm["pnr"] >= mc.MARGIN_TAG
    assert np.array_equal(s.tag_neurons_parallel(), tags_ref)
    ids = s.remove_false_positives()
    ids_ref, kept = mo.remove_false_positives(o.A, o.C, o.C_raw, o.S, o.kernel_pars, 5)
    assert np.array_equal(ids, ids_ref)
    oracle_set(kept)
    assert eng.counter("merge_trace_uploads") == n0, "a merge or tag call uploaded a K x T matrix although the engine held them"
    assert [g.tolist() for g in g_all] == [[0, 1]] and s.A.shape[1] == 11 - len(ids) and s.A_prev.shape[1] == 12
    check("after the merges")
    both("update_spatial_parallel"); both("update_temporal_parallel")
    check("spatial + temporal after the merges")
    for m in ("update_background_parallel", "update_spatial_parallel", "update_temporal_parallel"):
        both(m)
    check("iteration after the merges")
