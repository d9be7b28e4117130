"""float64 NumPy restatement of extract_DF_F_endoscope (@Sources2D/Sources2D.m:540-570) and of the three baseline estimators it calls.

  medfilt1_truncate    medfilt1(x, w, [], 2, 'truncate') -- a MathWorks function, restated from its documentation (PARITY UNPINNED): the window of sample k is
                       k - (w - 1)/2 .. k + (w - 1)/2 for odd w and k - w/2 .. k + w/2 - 1 for even w, clipped to the trace without padding; the median of what
                       remains, an even count giving the mean of the two middle samples
  running_percentile   utilities/running_percentile.m:74-121 (in the reference tree): window i - (ceil(w/2) - 1) .. i + floor(w/2) of the trace reflected at both
                       ends with the edge sample repeated (:76-78), pt = p w / 100 + 0.5 and the four branches of :90-104.  Its NaN bookkeeping is not restated:
                       a row with a non-finite value is NaN throughout (the deviation the engine documents)
  prctile              prctile(x, p, 2) -- a MathWorks function: the Hazen rule oracle.cnmfe_oracle.matlab_quantile restates (PARITY UNPINNED)

`pairs=True` makes an estimator also return the two order statistics (a, b) every output was formed from (a == b where it is a single one): what the GPU tests'
rounding bound 8 * 2^-52 * max(|a|, |b|) is built from."""
import numpy as np

from cnmfe_oracle import matlab_quantile


def _window_median(s):
    n = s.size
    a, b = s[(n - 1) // 2], s[n // 2]
    return (a if n % 2 else 0.5 * (a + b)), a, b


def medfilt1_truncate(x, w, pairs=False):
    x = np.asarray(x, dtype=np.float64)
    T, w = x.size, int(w)
    out, A, B = np.empty(T), np.empty(T), np.empty(T)
    for k in range(T):
        lo, hi = (k - (w - 1) // 2, k + (w - 1) // 2) if w % 2 else (k - w // 2, k + w // 2 - 1)
        out[k], A[k], B[k] = _window_median(np.sort(x[max(lo, 0):min(hi, T - 1) + 1]))
    return (out, A, B) if pairs else out


def reflect_pad(x, w):
    """running_percentile.m:76-78 without the trailing NaN: [x(ceil(w/2)-1 : -1 : 1), x, x(N : -1 : N-floor(w/2)+1)]"""
    x = np.asarray(x, dtype=np.float64)
    nl, nr = -(-w // 2) - 1, w // 2
    return np.concatenate([x[:nl][::-1], x, x[::-1][:nr]])


def running_percentile(x, w, p, pairs=False):
    x = np.asarray(x, dtype=np.float64)
    T, w = x.size, int(w)
    xp = reflect_pad(x, w)
    out, A, B = np.empty(T), np.empty(T), np.empty(T)
    pt = p * w / 100 + 0.5                                                  # :90
    for i in range(T):
        s = np.sort(xp[i:i + w])                                            # (tmp of :80, :120: the sorted window of sample i)
        if pt < 1:                                                          # :92-93
            a = b = y = s[0]
        elif pt > w:                                                        # :94-95
            a = b = y = s[w - 1]
        elif np.floor(pt) == np.ceil(pt):                                   # :96-97
            a = b = y = s[int(pt) - 1]
        else:                                                               # :98-103
            f = int(np.floor(pt))
            x0 = 100 * (f - 0.5) / w
            x1 = 100 * (f + 0.5) / w
            a, b = s[f - 1], s[f]
            y = a + (b - a) * ((p - x0) / (x1 - x0))
        out[i], A[i], B[i] = y, a, b
    return (out, A, B) if pairs else out


def prctile(x, p, pairs=False):
    x = np.asarray(x, dtype=np.float64)
    y = matlab_quantile(x, p / 100.0)
    if not pairs:
        return y
    s, n = np.sort(x), x.size
    r = (p / 100.0) * n + 0.5
    lo = 1 if r <= 1 else (n if r >= n else int(np.floor(r)))
    single = r <= 1 or r >= n or r == lo
    return y, s[lo - 1], s[lo - 1] if single else s[lo]


def baseline(Yf, df_prctile=50, df_window=None, pairs=False):
    """Df of Sources2D.m:546-566 for the K x T matrix Yf: (K,) without a window (df_window None / 0 / > T), (K, T) with one.  Rows with a non-finite value: NaN."""
    Yf = np.asarray(Yf, dtype=np.float64)
    K, T = Yf.shape
    win = bool(df_window) and df_window <= T
    shape = (K, T) if win else (K,)
    Df, A, B = np.full(shape, np.nan), np.full(shape, np.nan), np.full(shape, np.nan)
    for k in range(K):
        if not np.all(np.isfinite(Yf[k])):
            continue
        if not win:
            if df_prctile == 50:                                            # :549-550
                Df[k], A[k], B[k] = _window_median(np.sort(Yf[k]))
            else:                                                           # :552
                Df[k], A[k], B[k] = prctile(Yf[k], df_prctile, pairs=True)
        elif df_prctile == 50:                                              # :559
            Df[k], A[k], B[k] = medfilt1_truncate(Yf[k], df_window, pairs=True)
        else:                                                               # :563
            Df[k], A[k], B[k] = running_percentile(Yf[k], df_window, df_prctile, pairs=True)
    return (Df, A, B) if pairs else Df


def project(A, Ybg):
    """Yf = (A ./ sum(A.^2, 1))' * Ybg  (:545): A d x K (sparse or dense), Ybg d x T"""
    import scipy.sparse as sp
    A = sp.csc_matrix(A, dtype=np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        inv = 1.0 / np.asarray(A.power(2).sum(axis=0)).ravel()
        return (np.asarray((A.T @ np.asarray(Ybg, dtype=np.float64))) * inv[:, None])


def divide(X, Df):
    """C ./ Df as the engine returns it: (float)((double)C / Df), Df per row or per sample"""
    X = np.asarray(X, dtype=np.float32).astype(np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        return (X / (Df[:, None] if Df.ndim == 1 else Df)).astype(np.float32)


def extract_df_f(A, C, C_raw, Ybg, df_prctile=50, df_window=None):
    """[C_df, C_raw_df, Df] = extract_DF_F_endoscope(obj, Ybg)  (:540-570); Ybg d x T (or d1 x d2 x T)"""
    Ybg = np.asarray(Ybg)
    Ybg = Ybg.reshape(-1, Ybg.shape[-1], order="F")
    Df = baseline(project(A, Ybg), df_prctile, df_window)
    return divide(C, Df), divide(C_raw, Df), Df
