"""tests/df_oracle.py against brute force: every estimator of extract_DF_F_endoscope (Sources2D.m:540-570) is rebuilt from explicitly constructed windows and
NumPy's own order statistics, and the recording the GPU tests use is checked to make their division well conditioned and their accumulation cross patches."""
import numpy as np
import pytest
import scipy.sparse as sp

import df_cases
import df_oracle

T_ROW = 203
WINDOWS = [1, 2, 50, 51, T_ROW]


@pytest.fixture(scope="module")
def rows():
    rng = np.random.default_rng(11)
    g = rng.standard_normal((3, T_ROW)) * 7 + 300
    return np.concatenate([g, np.round(g[:1] / 4) * 4])                     # (the last row has ties)


def _clipped(x, k, w):
    lo, hi = (k - (w - 1) // 2, k + (w - 1) // 2) if w % 2 else (k - w // 2, k + w // 2 - 1)
    return np.array([x[j] for j in range(lo, hi + 1) if 0 <= j < x.size])


def _reflected(x, i, w):
    n = x.size
    idx = range(i - (-(-w // 2) - 1), i + w // 2 + 1)
    return np.array([x[-j - 1] if j < 0 else (x[2 * n - 1 - j] if j >= n else x[j]) for j in idx])


@pytest.mark.parametrize("w", WINDOWS)
def test_medfilt1_truncate_brute_force(rows, w):
    for x in rows:
        got = df_oracle.medfilt1_truncate(x, w)
        ref = np.array([np.median(_clipped(x, k, w)) for k in range(x.size)])
        assert np.array_equal(got, ref)
        if w == 1:
            assert np.array_equal(got, x)


@pytest.mark.parametrize("w", WINDOWS)
@pytest.mark.parametrize("p", [20, 30, 77.5])
def test_running_percentile_brute_force(rows, w, p):
    for x in rows:
        got = df_oracle.running_percentile(x, w, p)
        ref = np.array([np.percentile(_reflected(x, i, w), p, method="hazen") for i in range(x.size)])
        assert _reflected(x, 0, w).size == w
        assert np.allclose(got, ref, rtol=1e-14, atol=0)


@pytest.mark.parametrize("p", [0, 0.1, 20, 50, 99.9, 100])
def test_prctile_is_hazen(rows, p):
    for x in rows:
        y, a, b = df_oracle.prctile(x, p, pairs=True)
        assert np.isclose(y, np.percentile(x, p, method="hazen"), rtol=1e-14, atol=0)
        assert min(a, b) <= y <= max(a, b)
    assert df_oracle.prctile(rows[0], 0) == rows[0].min() and df_oracle.prctile(rows[0], 100) == rows[0].max()


def test_running_percentile_branches(rows):
    """running_percentile.m:92-97: pt < 1 -> the window's minimum, pt > w -> its maximum, integer pt -> s(pt) itself"""
    x, w = rows[0], 50
    win = [np.sort(_reflected(x, i, w)) for i in range(x.size)]
    y, a, b = df_oracle.running_percentile(x, w, 9, pairs=True)            # pt = 9 * 50 / 100 + 0.5 = 5
    assert np.array_equal(y, [s[4] for s in win]) and np.array_equal(a, b)
    assert np.array_equal(df_oracle.running_percentile(x, w, 0.5), [s[0] for s in win])       # pt = 0.75
    assert np.array_equal(df_oracle.running_percentile(x, w, 99.9), [s[-1] for s in win])     # pt = 50.45 > w
    y, a, b = df_oracle.running_percentile(x, w, 20, pairs=True)           # pt = 10.5: between s(10) and s(11)
    assert np.array_equal(a, [s[9] for s in win]) and np.array_equal(b, [s[10] for s in win])
    assert np.all((y >= a) & (y <= b))


def test_even_windows_are_mirror_images():
    """for even w medfilt1's window is k - w/2 .. k + w/2 - 1 and running_percentile's i - (w/2 - 1) .. i + w/2: one is the other on the reversed trace"""
    T, w = 40, 6
    x = np.arange(T, dtype=np.float64)
    for k in range(w, T - w):                                              # (away from the edges, where one clips and the other reflects)
        med = _clipped(x, k, w)
        run = _reflected(x, k, w)
        assert med[0] == k - w // 2 and med[-1] == k + w // 2 - 1
        assert run[0] == k - (w // 2 - 1) and run[-1] == k + w // 2
        rev = _reflected(x[::-1], T - 1 - k, w)
        assert np.array_equal(np.sort(rev), np.sort(med))
    x = np.random.default_rng(3).standard_normal(T)
    a = df_oracle.medfilt1_truncate(x, w)[w:T - w]
    b = df_oracle.running_percentile(x[::-1], w, 50)[::-1][w:T - w]
    assert np.allclose(a, b, rtol=1e-15, atol=1e-15)


def test_non_finite_rows_are_nan_throughout():
    Yf = np.random.default_rng(5).standard_normal((3, 80)) + 10
    Yf[1, 7] = np.nan
    Yf[2, :] = 0.0 * np.inf
    for p, w in [(50, None), (20, None), (50, 9), (20, 9)]:
        Df = df_oracle.baseline(Yf, p, w)
        assert np.all(np.isfinite(Df[0])) and np.all(np.isnan(Df[1])) and np.all(np.isnan(Df[2]))


def test_extract_df_f_shapes_and_division():
    rng = np.random.default_rng(9)
    d, K, T = 30, 3, 70
    A = sp.random(d, K, density=0.4, random_state=1, format="csc")
    C, R = rng.random((K, T)).astype(np.float32), rng.random((K, T)).astype(np.float32)
    Ybg = rng.random((d, T)) + 5
    C_df, R_df, Df = df_oracle.extract_df_f(A, C, R, Ybg, 50, None)
    assert Df.shape == (K,) and C_df.dtype == np.float32
    Yf = (A.toarray() / (A.toarray() ** 2).sum(axis=0)).T @ Ybg
    assert np.allclose(Df, np.median(Yf, axis=1), rtol=1e-13)
    assert np.array_equal(C_df, (C.astype(np.float64) / Df[:, None]).astype(np.float32))
    C_df, R_df, Df = df_oracle.extract_df_f(A, C, R, Ybg, 50, T + 1)       # a window longer than the recording means none (:546)
    assert Df.shape == (K,)
    C_df, R_df, Df = df_oracle.extract_df_f(A, C, R, Ybg, 30, 11)
    assert Df.shape == (K, T) and np.array_equal(R_df, (R.astype(np.float64) / Df).astype(np.float32))


@pytest.mark.parametrize("bg_ssub", [1, 2])
def test_fixture_is_well_conditioned(bg_ssub):
    """the recording of tests/df_cases.py: min_k |Df| >= 0.05 median_k |Df| for every setting the GPU tests divide by, and a neuron in two patches"""
    f, Y = df_cases.recording()
    o = df_cases.oracle_after_one_iteration(f, Y, bg_ssub)
    Ybg = o.reconstruct_background().reshape(df_cases.D1 * df_cases.D2, df_cases.T, order="F")
    A = sp.csc_matrix(o.A)
    Yf = df_oracle.project(A, Ybg)
    for p, w in df_cases.E2E_SETTINGS:
        Df = np.abs(df_oracle.baseline(Yf, p, w))
        assert np.all(np.isfinite(Df))
        assert Df.min() >= 0.05 * np.median(Df), (p, w, Df.min(), np.median(Df))
    assert max(len(s) for s in df_cases.patches_of_neurons(A)) >= 2
