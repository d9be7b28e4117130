"""Float64 restatement of the closing calls of demos/demo_large_data_1p.m, for the tests of cnmf_e_amd's orderROIs / demixed_frames / show_demixed_video:

  the six panels of @Sources2D/show_demixed_video.m:70-81,94-127 from OracleSources2D.reconstruct_background (oracle/cnmfe_oracle.py),
  MATLAB's uint16() conversion, the criteria of orderROIs (@Sources2D/Sources2D.m:573-653) with MATLAB's sort rule, and the display ranges of :36-57.

Nothing here is imported by the product; the product's own statements (cnmf_e_amd/hostops.py) are tested AGAINST these."""
import numpy as np
import scipy.sparse as sp


def matlab_uint16(x):
    """uint16(x): round to the nearest integer, halves away from zero; saturate to [0, 65535]; NaN -> 0"""
    x = np.asarray(x, dtype=np.float64)
    sat = np.clip(np.where(np.isnan(x), 0.0, x), -1.0, 65536.0)              # (saturation first: nothing beyond it changes the result)
    up = np.floor(sat + 0.5)                                                 # for sat >= 0 halves go up = away from zero; negative values end at 0 anyway
    return np.clip(up, 0.0, 65535.0).astype(np.uint16)


def rounding_distance(x):
    """distance of every value to the nearest boundary of uint16()'s rounding (k + 0.5), Inf where the conversion saturates anyway"""
    x = np.asarray(x, dtype=np.float64)
    dist = np.abs((x - 0.5) - np.round(x - 0.5))
    return np.where((x < -0.5) | (x > 65535.5), np.inf, dist)


def mixed_double(A, CC, col, amp_ac):
    """Y_mixed(:, :, m) * 2 / amp_ac * 65536 before the conversion (show_demixed_video.m:79-81), d x n x 3 float64"""
    A = sp.csr_matrix(A).astype(np.float64)
    CC = np.asarray(CC, dtype=np.float64)
    col = np.asarray(col, dtype=np.float64)
    out = np.zeros((A.shape[0], CC.shape[1], 3))
    for m in range(3):
        out[:, :, m] = np.asarray(A @ (col[:, m][:, None] * CC)) * 2 / amp_ac * 65536
    return out


def panels_from(raw, bg, A, CC, col, amp_ac):
    """raw, bg: d x n float64; A: d x K; CC: K x n; col: K x 3 -> dict of the six panels (float64; mixed uint16 d x n x 3, mixed_double the values before uint16())"""
    raw = np.asarray(raw, dtype=np.float64); bg = np.asarray(bg, dtype=np.float64)
    A = sp.csr_matrix(A).astype(np.float64)
    ac = np.asarray(A @ np.asarray(CC, dtype=np.float64)) if A.shape[1] else np.zeros_like(raw)      # :113
    md = mixed_double(A, CC, col, amp_ac) if A.shape[1] else np.zeros(raw.shape + (3,))
    return dict(raw=raw, bg=bg, signal=raw - bg, denoised=ac, residual=raw - bg - ac, mixed=matlab_uint16(md), mixed_double=md)      # :94, :101, :107, :113, :120, :81


def panels(o, frames, CC, col, amp_ac, Ybg=None):
    """the panels of the 0-based frames `frames` of an OracleSources2D state: raw is the video itself, bg its reconstruct_background()"""
    d = o.d1 * o.d2
    frames = np.asarray(frames)
    Ybg = o.reconstruct_background() if Ybg is None else Ybg
    raw = np.asarray(o.Y, dtype=np.float64).reshape(d, o.T, order="F")[:, frames]
    bg = Ybg.reshape(d, o.T, order="F")[:, frames]
    return panels_from(raw, bg, o.A, np.asarray(CC, dtype=np.float64)[:, frames], col, amp_ac)


def default_amp_ac(A, CC):
    """median(max(obj.A, [], 1)' .* max(CC, [], 2)) * 2  (:37)"""
    A = sp.csc_matrix(A).astype(np.float64)
    amax = np.asarray(A.max(axis=0).todense()).ravel()
    return float(np.median(amax * np.asarray(CC, dtype=np.float64).max(axis=1)) * 2)


def ranges(amp_ac, raw_samples=None, range_ac=None, range_Y=None, multi_factor=None, quantile=None):
    """:36-57, statement by statement; `quantile(x, p)` = MATLAB's quantile"""
    range_ac = amp_ac * np.array([0.01, 1.01]) if range_ac is None else np.asarray(range_ac, dtype=np.float64)
    range_res = range_ac - np.mean(range_ac)
    mf_exists = multi_factor is not None
    if range_Y is None:
        if not mf_exists:
            temp = quantile(raw_samples, [0.01, 0.98])
            multi_factor = np.ceil(np.diff(temp)[0] / np.diff(range_ac)[0]); mf_exists = True
        else:
            temp = quantile(raw_samples, [0.01])
        center_Y = temp[0] + multi_factor * amp_ac / 2
        range_Y = center_Y + range_res * multi_factor
    range_Y = np.asarray(range_Y, dtype=np.float64)
    if not mf_exists:
        multi_factor = np.round(np.diff(range_Y)[0] / np.diff(range_ac)[0])
        range_Y = (range_res - range_res[0]) * multi_factor + range_Y[0]
    return dict(range_ac=range_ac, range_res=range_res, range_Y=range_Y, multi_factor=float(multi_factor))


# ---- orderROIs ------------------------------------------------------------------------------------------------------
def stable_sort_brute(x, descend=False):
    """MATLAB's sort order by insertion: an element moves in front of its predecessor only if it is strictly smaller (ascend) / larger (descend); NaN counts as the
    largest value in both directions (last ascending, first descending); equal elements and NaNs keep their order"""
    x = [float(v) for v in np.asarray(x, dtype=np.float64).ravel()]

    def before(a, b):                                                        # must a go in front of b?
        an, bn = a != a, b != b
        if descend:
            return (an and not bn) or (not an and not bn and a > b)
        return (bn and not an) or (not an and not bn and a < b)
    order = []
    for i, v in enumerate(x):
        j = len(order)
        while j > 0 and before(v, x[order[j - 1]]):
            j -= 1
        order.insert(j, i)
    return np.array(order, dtype=np.int64)


def order_stats(C, C_raw):
    """the seven per-trace statistics of cnmfe_trace_order_stats in float64 NumPy"""
    C = np.asarray(C, dtype=np.float64); R = np.asarray(C_raw, dtype=np.float64)
    dd = 1 if C.shape[1] > 1 else 0
    return np.stack([C.mean(axis=1), C.var(axis=1, ddof=dd), (R - C).var(axis=1, ddof=dd), C.max(axis=1), np.sqrt((R ** 2).sum(axis=1)), np.abs(R).sum(axis=1),
                     R.max(axis=1)], axis=1)


def order_criterion(name, A, C, C_raw, kernel_pars=None, deconv_flag=True, neuron_sn=None):
    """(values, descend) of Sources2D.m:583-639"""
    A = sp.csc_matrix(A).astype(np.float64)
    C = np.asarray(C, dtype=np.float64); R = np.asarray(C_raw, dtype=np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        if name.lower() == "decay_time":
            g = np.asarray(kernel_pars, dtype=np.float64).ravel()
            return -1.0 / np.log(np.maximum(g, 0.0)), False                  # ar2exp of an AR(1) coefficient: tau_d = -1 / log(g)
        if name == "mean":
            v = C.mean(axis=1) * np.asarray(A.sum(axis=0)).ravel()
            return (v if deconv_flag else v / np.asarray(neuron_sn, dtype=np.float64).ravel()), True
        if name == "sparsity_spatial":
            return np.sqrt(np.asarray(A.power(2).sum(axis=0)).ravel()) / np.asarray(abs(A).sum(axis=0)).ravel(), False
        if name == "sparsity_temporal":
            return np.sqrt((R ** 2).sum(axis=1)) / np.abs(R).sum(axis=1), True
        if name.lower() == "pnr":
            return C.max(axis=1) / (R - C).std(axis=1, ddof=1), True
        return C.var(axis=1, ddof=1) / (R - C).var(axis=1, ddof=1), True


def order_rois(name, A, C, C_raw, **kw):
    val, desc = order_criterion(name, A, C, C_raw, **kw)
    return stable_sort_brute(val, desc), val


def margin(val):
    """smallest relative gap between two neighbours of the sorted finite values (ties and NaN / Inf aside: the caller names them)"""
    v = np.sort(np.asarray(val, dtype=np.float64)[np.isfinite(val)])
    gaps = np.diff(v) / np.maximum(np.abs(v[1:]), np.abs(v[:-1]))
    gaps = gaps[gaps > 0]
    return float(gaps.min()) if gaps.size else np.inf
