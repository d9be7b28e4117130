"""Host self-check of tests/deconv_branch_cases.py, on the oracle alone (no engine, no GPU): every row reaches the branch its tag names and is
well-conditioned, so that tests/test_gpu_deconv_branches.py may ask the engine for the oracle's spike support sample by sample.

Well-conditioned: the oracle rerun with sn * (1 +- 1e-6) keeps the spike support and moves g by < 1e-5 and C by < 1e-5 relative -- 10x the perturbation,
which itself is 20x the 5e-8 the engine's sn is off the oracle's (tests/test_gpu_parity.py::test_deconv_temporal_parity).  A row that fails is reseeded in the
case tables; nothing here skips or excludes a row, and the table's size is asserted."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import deconv_branch_cases as dbc
import oasis_oracle as oo

PERTURB, BOUND = 1e-6, 1e-5


def raw_estimate(y, sn):
    """estimate_time_constant.m:40-49 before the |g| > 1 and g < 0 rules"""
    y = np.asarray(y, np.float64)
    yn = y - y.mean()
    xc = np.array([yn[k:] @ yn[:y.size - k] for k in range(7)]) / y.size
    A = xc[:6].copy(); A[0] -= sn ** 2
    return float(A @ xc[1:7] / (A @ A))


def row(y, opts, f=1.0):
    """deconvTemporal.m:45-51 of one row with the noise level scaled by f: (c, s, b, g)"""
    y = np.asarray(y, np.float64)
    o = dict(opts); maxIter = int(o.pop("maxIter", 10))
    return oo.deconvolveCa_ar1_foopsi(y, oo.GetSn(y) * f, None, maxIter=maxIter, **o)


def conditioning(y, opts):
    """(support kept, |dg|, rel dC), the worst over sn * (1 - 1e-6) and sn * (1 + 1e-6)"""
    c, s, b, g = row(y, opts)
    same, dg, dc = True, 0.0, 0.0
    for f in (1 - PERTURB, 1 + PERTURB):
        c2, s2, b2, g2 = row(y, opts, f)
        same &= bool(np.array_equal(s > 0, s2 > 0))
        dg = max(dg, abs(g - g2))
        dc = max(dc, float(np.linalg.norm(c2 - c) / max(np.linalg.norm(c), 1e-30)))
    return same, dg, dc


def pool_lengths(s):
    """lengths of the pools of a solution: the stretches between spikes (the first pool starts at frame 0)"""
    starts = np.r_[0, np.nonzero(s[1:] > 0)[0] + 1]
    return np.diff(np.r_[starts, s.size])


def test_table_size():
    cases = dbc.all_cases()
    assert len(cases) == dbc.N_CASES == 61
    assert sum(Y.shape[0] for _, Y, _, _ in cases) == dbc.N_ROWS == 254
    assert len({n for n, _, _, _ in cases}) == len(cases)
    for name, Y, opts, tags in cases:
        assert Y.dtype == np.float32 and Y.ndim == 2 and len(tags) == Y.shape[0] and 64 <= Y.shape[1] <= 600, name
    assert sorted({Y.shape[1] for n, Y, _, _ in cases if n.startswith("options")}) == [64, 65, 127, 129, 257, 600]
    assert len(dbc.OPTION_ROWS) == 8 and len(dbc.POOL_P) == 13


@pytest.mark.parametrize("case", dbc.all_cases(), ids=lambda c: c[0])
def test_rows_reach_their_branch_and_are_well_conditioned(case):
    name, Y, opts, tags = case
    gmax = np.exp(-1.0 / opts["max_tau"])
    Cr, Crawr, Sr, parsr, snr = dbc.reference(name)
    for k, tag in enumerate(tags):
        y = Y[k].astype(np.float64)
        if tag == "nan":
            assert np.isnan(y).sum() == 1
            assert not Cr[k].any() and not Sr[k].any() and not Crawr[k].any() and parsr[k] == 0
            continue
        sn = oo.GetSn(y)
        g_raw = raw_estimate(y, sn)
        g0 = oo.estimate_time_constant_ar1(y, sn)
        if tag == "giveup":
            assert abs(g_raw) > 1.0 and g0 is None, (name, k, g_raw)
            assert parsr[k] == 0 and not Sr[k].any() and np.array_equal(Cr[k], Crawr[k]) and np.array_equal(Cr[k], y)
            continue                                            # (nothing depends on sn beyond the sign of |g| - 1: g_raw is 3e-3 or more beyond it)
        if tag == "restart":
            assert g0 > gmax and opts["optimize_b"], (name, k, g0)
            assert parsr[k] == pytest.approx(g0, abs=1e-12)     # the re-estimate on the same row with the same sn
        elif tag == "update_g":
            assert g0 > gmax and not opts["optimize_b"], (name, k, g0)
            assert abs(parsr[k] - g0) > 1e-3, (name, k, parsr[k], g0)      # update_g moved it: the GPU test tells the two branches apart by this
        elif tag == "rule015":
            assert -0.9 < g_raw < -0.05 and g0 == 0.15, (name, k, g_raw)
        elif tag.startswith("ties"):
            v0, v1, n0, n1 = dbc.q15_pair(Y[k])
            assert n0 >= 10 and n1 >= 10, (name, k, n0, n1)
            if tag == "ties_negative":
                assert Y[k].max() < 0
            if tag == "ties_straddle":
                assert v0 < 0 < v1
        elif tag == "pools":
            P = dbc.POOL_P[k]
            ln = pool_lengths(Sr[k])
            if P < 6:
                assert (ln < 6).sum() >= 10, (name, k, ln)      # events denser than six samples: the one-sample stretch of the wave pass
            elif P >= 30:
                assert P in ln, (name, k, ln)
        same, dg, dc = conditioning(y, opts)
        assert same, (name, k, "spike support moves with sn * (1 +- 1e-6): reseed this row")
        assert dg < BOUND and dc < BOUND, (name, k, dg, dc)


def test_pool_lengths_cover_the_task_boundaries():
    """pools exactly at and beside one, two and three tasks of DTK = 31 samples, and runs longer than a wave (64 lanes)"""
    seen = set()
    for name, Y, opts, tags in dbc.all_cases():
        if name.startswith("pools"):
            Sr = dbc.reference(name)[2]
            for k in range(Y.shape[0]):
                seen |= set(pool_lengths(Sr[k]).tolist())
    assert dbc.DTK == 31 and {31, 62, 63, 64, 65, 93} <= seen, sorted(seen)
