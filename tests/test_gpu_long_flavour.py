"""The long flavour of the session and trace kernels (k_seed_stats_long, k_peel_trace_stats_long, k_trace_diff_spikes_long, k_trace_tags_long: the trace in
global memory, LDS the Welch transform alone) against the LDS flavour at frame counts both can take: option trace_long = 1 routes every call to the long
flavour, and every output must equal the default run's BIT FOR BIT -- same 256 threads, strides, fma order and get_sn instantiation.  trace_long = 0 must equal
a run that never set the option.  Also the envelope: 64 <= frames <= WELCH_TMAX = 147456."""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import long_cases as lc
import merge_cases as mc
import oasis_oracle as oo

pytestmark = pytest.mark.gpu


def _seed_case(name):
    from test_gpu_seed_images import CASES
    return CASES[name]


@pytest.mark.parametrize("name", ["A", "D", "B"])          # four blocks with halo; detrend; 113 taps
def test_seed_images_bit_equal(name):
    c = _seed_case(name)
    Cn0, PNR0, Sn0 = lc.seed_images_run(c, None)
    Cn1, PNR1, Sn1 = lc.seed_images_run(c, 1)
    assert np.all(np.isfinite(Cn0)) and np.all(PNR0 > 0) and all(np.all(v[2] > 0) for v in Sn0.values())
    assert np.array_equal(Cn0, Cn1) and np.array_equal(PNR0, PNR1)
    assert lc.equal_tree(Sn0, Sn1) is None                   # per patch: the open's (Cn, PNR, Sn) of the block
    if name == "A":
        Cnz, PNRz, Snz = lc.seed_images_run(c, 0)            # (trace_long = 0 is a run that never set the option)
        assert np.array_equal(Cn0, Cnz) and np.array_equal(PNR0, PNRz) and lc.equal_tree(Sn0, Snz) is None


@pytest.mark.parametrize("name", ["A", "C", "D"])          # four blocks; detrend; deconvolution
def test_greedy_steps_bit_equal(name):
    """forced seeds, the step observer: every step's corr, ci, ai, stats and PNR / Cn boxes, then Cn, PNR, A, C, C_raw, S"""
    a, b = lc.greedy_run(name, None), lc.greedy_run(name, 1)
    nsteps = sum(len(v) for v in a["steps"].values())
    assert nsteps >= 2 and a["A"].any()
    assert any(kind == "extract" and "sn_ci" in d["stats"] and {"corr", "ci", "ai"} <= set(d) for v in a["steps"].values() for kind, d in v)
    assert lc.equal_tree(a, b) is None, lc.equal_tree(a, b)


def test_residual_second_pass_bit_equal():
    a, b = lc.residual_run("Q", None), lc.residual_run("Q", 1)
    assert a["A"].shape[1] > 2 and sum(len(v) for v in a["steps"].values()) >= 2          # the pass found the withheld neurons
    assert lc.equal_tree(a, b) is None, lc.equal_tree(a, b)


def _trace_calls(trace_long):
    X, Y, Z = mc.traces(17, 403), mc.traces(17, 403, seed=6), mc.traces(17, 403, seed=7)
    eng = lc.engine(trace_long)
    try:
        eng.traces_load(X, Y, np.maximum(Z, 0))
        tags = eng.trace_tags()
        sn, S_ = eng.trace_diff_spikes(Y, want=True)
        return dict(tags=tags, sn=sn, S_=S_)
    finally:
        eng.close()


def test_trace_calls_bit_equal():
    a, b, z = _trace_calls(None), _trace_calls(1), _trace_calls(0)
    assert (a["sn"] > 0).sum() == 16 and a["sn"][15] == 0 and a["S_"].any() and np.all(a["tags"][:, 2] > 0)       # (row K - 2 is constant: its differences are 0)
    assert lc.equal_tree(a, b) is None, lc.equal_tree(a, b)
    assert lc.equal_tree(a, z) is None


def test_envelope():
    """a trace call beyond WELCH_TMAX is refused with CNMFE_EUNSUPPORTED and leaves the context usable; the seed images' other refusals stay"""
    from cnmf_e_amd._lib import CnmfeError
    from cnmf_e_amd.sources2d import PatchedVideo, seed_psf
    eng = lc.engine()
    try:
        X = np.random.default_rng(0).standard_normal((2, 150000)).astype(np.float32)
        with pytest.raises(CnmfeError, match="error -5") as ei:
            eng.trace_diff_spikes(X, want=True)
        assert "WELCH_TMAX" in str(ei.value)
        eng.traces_load(X, X, None)
        with pytest.raises(CnmfeError, match="error -5"):
            eng.trace_tags()
        sn, S_ = eng.trace_diff_spikes(X[:, :147456], want=True)            # the largest count taken
        ref = np.array([oo.GetSn(np.r_[np.diff(x[:147456].astype(np.float64)), 0.0]) for x in X])
        assert np.all(np.abs(sn - ref) <= lc.SN_TOL * ref) and S_.shape == (2, 147456)
        d1, d2, T = 24, 20, 80
        video = PatchedVideo(d1, d2, T, [d1, d2], 3, eng)
        video.upload_from_full(np.random.default_rng(0).standard_normal((T, d1 * d2)).astype(np.float32))
        psf = seed_psf(1.5, 7, True)
        for kw in (dict(nframes=40), dict(frame0=4, nframes=64)):
            with pytest.raises(CnmfeError, match="error -5"):
                eng.seed_images(0, psf, **kw)
        Cn, PNR = eng.seed_images(0, psf)
        assert np.all(np.isfinite(Cn)) and np.all(PNR > 0)
    finally:
        eng.close()
