"""Host-side image operations on single footprints: the optional branches around the spatial update.

  search_method = 'dilate'        utilities/determine_search_location.m:89-94  (threshold_components.m:1-63 + imdilate)
  spatial_constraints.circular    endoscope/circular_constraints.m:1-55   (also Sources2D.compactSpatial)
  trimSpatial                     @Sources2D/Sources2D.m:942-965

CNMFSetParms.m sets search_method 'ellipse' and circular false, but the demos do not all leave them there: demo_batch_1p.m:19 and demo_sfn_2018.m:19 set
with_dendrites = true, which selects search_method = 'dilate', and demo_large_data_1p.m:132 / demo_sfn_2018.m:130 / demo_endoscope.m:135-136 call
compactSpatial (circular_constraints per column) and trimSpatial.  An engine that declares supports_image_ops runs these on the device (csrc/footprint_ops.hpp) and
EQUALS the functions here, which remain the statement of the arithmetic, the path of every other engine, and the path of a column whose box exceeds
Engine.IMAGE_OPS_MAX_BOX.  Each works on one d1 x d2 image per neuron.  The Image
Processing Toolbox calls are written with scipy.ndimage under the toolbox's documented border rules: medfilt2 pads with zeros, imdilate
with -Inf, imerode with +Inf; bwlabel(., 4) / bwlabeln(., 8) are 4- / 8-connected; strel('disk', R, 0) is the exact disc x^2 + y^2 <= R^2.

Further down: the host halves of the greedy initialisation, of the merges and of the closing calls (orderROIs' sort rule, show_demixed_video's ranges and montage).
"""
from __future__ import annotations

import numpy as np
import scipy.ndimage as ndi
import scipy.sparse as sp

SQUARE3 = np.ones((3, 3), dtype=bool)
CROSS4 = np.array([[0, 1, 0], [1, 1, 1], [0, 1, 0]], dtype=bool)


def strel_disk(radius):
    """strel('disk', R, 0): every pixel whose centre is no further than R from the origin"""
    r = int(radius)
    y, x = np.mgrid[-r:r + 1, -r:r + 1]
    return (x * x + y * y) <= radius * radius


def medfilt2(img, size=(3, 3)):
    """medfilt2(img, [m n]): median of the m x n neighbourhood, the image padded with zeros"""
    return ndi.median_filter(img, size=tuple(int(s) for s in size), mode="constant", cval=0.0)


def imclose(bw, se):
    """imclose = imerode(imdilate(bw, se), se): the dilation sees -Inf (false) outside the image, the erosion +Inf (true)"""
    return ndi.binary_erosion(ndi.binary_dilation(bw, structure=se, border_value=0), structure=se, border_value=1)


def threshold_components(A, d1, d2, nb=1, nrgthr=0.99, medw=(3, 3), clos_op=None):
    """Ath = threshold_components(A, options) (threshold_components.m:20-62): per component median filter, keep the pixels holding `nrgthr`
    of the energy, close, keep the 8-connected component with the most energy (values of the FILTERED image).  The last `nb` columns are
    copied unchanged (:22,25)."""
    A = sp.csc_matrix(A)
    d, nr = A.shape
    clos_op = SQUARE3 if clos_op is None else np.asarray(clos_op, dtype=bool)
    rows, cols, vals = [], [], []
    for i in range(nr):
        col = A.getcol(i)
        if i >= nr - nb:                                                   # :22
            rows.append(col.indices); cols.append(np.full(col.nnz, i)); vals.append(col.data.astype(np.float64))
            continue
        img = medfilt2(np.asarray(col.todense(), dtype=np.float64).reshape(d1, d2, order="F"), medw)   # :28
        a = img.reshape(-1, order="F")
        e = a * a
        order = np.argsort(e, kind="stable")                               # :31 (sort is stable)
        cs = np.cumsum(e[order])                                           # :32
        above = np.nonzero(cs > (1.0 - nrgthr) * cs[-1])[0]                # :33
        bw = np.zeros(d, dtype=bool)
        if above.size:
            bw[order[above[0]:]] = True                                    # :35
        bw = imclose(bw.reshape(d1, d2, order="F"), clos_op)               # :37
        lab, num = ndi.label(bw, structure=SQUARE3)                        # :39 (8-connected)
        if num == 0:
            continue                                                       # :52 (nothing is written)
        nrg = ndi.sum(img * img, lab, index=np.arange(1, num + 1))         # :43-45
        keep = np.nonzero((lab == 1 + int(np.argmax(nrg))).reshape(-1, order="F"))[0]   # :46-47
        rows.append(keep); cols.append(np.full(keep.size, i)); vals.append(a[keep])      # :49-50,55-56
    if not rows:
        return sp.csc_matrix((d, nr), dtype=np.float64)
    return sp.csc_matrix((np.concatenate(vals), (np.concatenate(rows), np.concatenate(cols))), shape=(d, nr))


def search_location_dilate(A, d1, d2, se, nb=1, nrgthr=0.99, medw=(3, 3), clos_op=None):
    """IND = determine_search_location(A, 'dilate', params) (determine_search_location.m:51-56,89-98): threshold, then grow every
    footprint by the structuring element `se`."""
    A = sp.csc_matrix(A, dtype=np.float64).copy()
    d, nr = A.shape
    ind_empty = np.asarray(A.sum(axis=0)).ravel() == 0                     # :52
    if ind_empty.any():                                                    # :53-55
        A = A.tolil(); A[0, np.nonzero(ind_empty)[0]] = 1.0; A = A.tocsc()
    Ath = threshold_components(A, d1, d2, nb, nrgthr, medw, clos_op)       # :90
    se = np.asarray(se, dtype=bool)
    rows, cols = [], []
    for i in range(nr):
        if ind_empty[i]:                                                   # :97-98
            continue
        img = np.asarray(Ath.getcol(i).todense()).reshape(d1, d2, order="F") > 0
        # imdilate of a non-negative image by a flat element is > 0 exactly where the dilated support is (:92-93)
        keep = np.nonzero(ndi.binary_dilation(img, structure=se, border_value=0).reshape(-1, order="F"))[0]
        rows.append(keep); cols.append(np.full(keep.size, i))
    if not rows:
        return sp.csc_matrix((d, nr), dtype=bool)
    r, c = np.concatenate(rows), np.concatenate(cols)
    return sp.csc_matrix((np.ones(r.size, dtype=bool), (r, c)), shape=(d, nr))


def circular_constraints(img):
    """img = circular_constraints(img) (circular_constraints.m:8-55): inside the bounding box of the non-zeros, zero the pixels below a
    third of the peak whose gradient points away from the peak, keep the 4-connected component of the peak grown by one pixel, and median
    filter."""
    img = np.array(img, dtype=np.float64)
    r, c = np.nonzero(img)
    if r.size == 0:                                                        # :9-11
        return img
    rmin, rmax, cmin, cmax = r.min(), r.max(), c.min(), c.max()
    if rmax - rmin < 1 or cmax - cmin < 1:                                 # :17-19
        return img
    sub = img[rmin:rmax + 1, cmin:cmax + 1].copy()                         # :53 (the recursive call sees the cropped image)
    nr, nc = sub.shape
    ind_max = int(np.argmax(sub.reshape(-1, order="F")))                   # :30 (first maximum, column-major)
    vmax = sub.reshape(-1, order="F")[ind_max]
    y0, x0 = ind_max % nr, ind_max // nr                                   # :31 (0-based; only differences are used)
    y, x = np.mgrid[:nr, :nc]                                              # :32
    fy, fx = np.gradient(sub)                                              # :33 gradient(): central differences, one-sided at the edges
    ind = ((fx * (x0 - x) + fy * (y0 - y)) < 0) & (sub < vmax / 3.0)       # :34
    sub[ind] = 0                                                           # :35
    lab, _ = ndi.label(sub != 0, structure=CROSS4)                         # :39
    keep = ndi.binary_dilation(lab == lab[y0, x0], structure=SQUARE3, border_value=0)   # :40
    sub[~keep] = 0                                                         # :41
    img[rmin:rmax + 1, cmin:cmax + 1] = medfilt2(sub)                      # :42,54
    return img


def circular_constraints_columns(A, d1, d2):
    """post_process_spatial.m:29-31 for every column of a sparse d x K matrix"""
    A = sp.csc_matrix(A)
    rows, cols, vals = [], [], []
    for k in range(A.shape[1]):
        col = A.getcol(k)
        if col.nnz == 0:
            continue
        out = circular_constraints(np.asarray(col.todense()).reshape(d1, d2, order="F")).reshape(-1, order="F")
        nz = np.nonzero(out)[0]
        rows.append(nz); cols.append(np.full(nz.size, k)); vals.append(out[nz].astype(A.dtype))
    if not rows:
        return sp.csc_matrix(A.shape, dtype=A.dtype)
    out = sp.csc_matrix((np.concatenate(vals), (np.concatenate(rows), np.concatenate(cols))), shape=A.shape)
    out.sort_indices()
    return out


def trim_spatial(A, d1, d2, thr=0.01, sz=5, min_pixel=0):
    """ind_small = obj.trimSpatial(thr, sz) (@Sources2D/Sources2D.m:942-965) for every column of a sparse d x K matrix: open with a sz x sz square, threshold at
    thr * max(ai), keep the 4-connected component that holds the maximum of the OPENED image (nothing is zeroed when the opening removed everything: l is all
    zero); ind_small(m) = sum(ai > 0) < min_pixel.  Returns (the trimmed matrix, ind_small).  An even sz is refused: the toolbox's origin of an even element is a
    rule of its own that nothing here needs."""
    sz = int(sz)
    if sz < 1 or sz > 9 or sz % 2 == 0:
        raise ValueError("trim_spatial: sz = %d; the square's side is odd, 1 .. 9" % sz)
    A = sp.csc_matrix(A)
    K = A.shape[1]
    ind_small = np.zeros(K, dtype=bool)
    rows, cols, vals = [], [], []
    for k in range(K):
        col = A.getcol(k)
        img = np.asarray(col.todense(), dtype=np.float64).reshape(d1, d2, order="F")
        if col.nnz:
            ai_open = ndi.maximum_filter(ndi.minimum_filter(img, size=sz, mode="constant", cval=np.inf), size=sz, mode="constant", cval=-np.inf)   # :951
            lab, _ = ndi.label(ai_open > img.max() * thr, structure=CROSS4)                                                                     # :953-954
            ind_max = int(np.argmax(ai_open.reshape(-1, order="F")))                                                                            # :955
            img[lab != lab[ind_max % d1, ind_max // d1]] = 0                                                                                    # :957
        ind_small[k] = np.count_nonzero(img > 0) < min_pixel                                                                                    # :958
        nz = np.nonzero(img.reshape(-1, order="F"))[0]
        rows.append(nz); cols.append(np.full(nz.size, k)); vals.append(img.reshape(-1, order="F")[nz].astype(A.dtype))
    out = sp.csc_matrix((np.concatenate(vals), (np.concatenate(rows), np.concatenate(cols))), shape=A.shape) if K else sp.csc_matrix(A.shape, dtype=A.dtype)
    out.sort_indices()
    return out, ind_small


# --------------------------------------------------------------------------------------
# greedy initialisation (Sources2D.initComponents_parallel): the work on single block images and single traces around the device's peel session
#   endoscope/greedyROI_endoscope.m:62-164,193-216,262-311,339-410,447-463   the search loop
#   endoscope/extract_ac.m:60-107                                             constraints, minimum size, baseline
#   endoscope/connectivity_constraint.m, endoscope/remove_baseline.m, OASIS_matlab/functions/estimate_baseline_noise.m, fit_gauss1.m
# Everything is float64.  Toolbox rules used: ordfilt2 pads with zeros and centres an even domain at floor((n + 1) / 2); quantile places the sorted samples at
# the probabilities (i - 0.5) / n and interpolates linearly, clamped to the extremes; hist(y, centres) counts between the mid-points of the centres with open
# outer bins (a value on a mid-point goes to the lower bin); imopen erodes with +Inf and dilates with -Inf outside the image.
# --------------------------------------------------------------------------------------
def matlab_quantile(x, p):
    x = np.sort(np.asarray(x, dtype=np.float64).ravel())
    n = x.size
    pos = np.clip(np.asarray(p, dtype=np.float64) * n + 0.5, 1.0, float(n))   # 1-based position among the sorted samples
    lo = np.floor(pos).astype(np.int64)
    hi = np.minimum(lo + 1, n)
    return x[lo - 1] + (pos - lo) * (x[hi - 1] - x[lo - 1])


def hist_centres(y, centres):
    """nums = hist(y, centres)"""
    centres = np.asarray(centres, dtype=np.float64)
    mids = 0.5 * (centres[:-1] + centres[1:])
    return np.bincount(np.searchsorted(mids, np.asarray(y, dtype=np.float64).ravel(), side="left"), minlength=centres.size).astype(np.float64)


def fit_gauss1(x, y, thr=0.1, maxIter=5, mu_fix=False):
    """[mu, sig, A] = fit_gauss1(x, y, thr, maxIter, mu_fix) (fit_gauss1.m:21-87): iteratively re-weighted least squares on log y = p0 + p1 x + p2 x^2
    over the points above thr * max(y) (Guo 2011)"""
    x = np.asarray(x, dtype=np.float64).ravel(); y = np.asarray(y, dtype=np.float64).ravel()
    ind = y > y.max() * thr                                                # :35
    x = x[ind]; y = y[ind]
    x2 = x * x; x3 = x2 * x; x4 = x2 * x2
    y2 = y * y; logy = np.log(y); y2logy = y2 * logy
    with np.errstate(all="ignore"):
        for _ in range(int(maxIter)):
            if mu_fix:                                                     # :50-64
                M = np.array([[y2.sum(), x2 @ y2], [x2 @ y2, x4 @ y2]])
                b = np.array([y2logy.sum(), x2 @ y2logy])
            else:                                                          # :66-77
                M = np.array([[y2.sum(), x @ y2, x2 @ y2], [x @ y2, x2 @ y2, x3 @ y2], [x2 @ y2, x3 @ y2, x4 @ y2]])
                b = np.array([y2logy.sum(), x @ y2logy, x2 @ y2logy])
            try:
                p = np.linalg.solve(M, b)
            except np.linalg.LinAlgError:
                p = np.full(b.size, np.nan)
            logy = p[0] + p[1] * x2 if mu_fix else p[0] + p[1] * x + p[2] * x2
            y = np.exp(logy); y2 = y * y; y2logy = y2 * logy
        if mu_fix:
            return 0.0, float(np.sqrt(-0.5 / p[1])), float(np.exp(p[0]))
        return float(-p[1] / 2 / p[2]), float(abs(np.sqrt(-0.5 / p[2] + 0j))), float(np.exp(p[0] - 0.25 * p[1] ** 2 / p[2]))


def estimate_baseline_noise(y, bmin=-np.inf):
    """[b, sn] = estimate_baseline_noise(y, bmin) (estimate_baseline_noise.m:18-35): a Gaussian fitted to the histogram of the trace around its mode"""
    y = np.asarray(y, dtype=np.float64).ravel()
    temp = matlab_quantile(y, np.arange(11) / 10.0)                        # :18
    dbin = max(np.diff(temp).min() / 3.0, (temp.max() - temp.min()) / 1000.0)   # :19
    if not dbin > 0:                                                       # :24-28 (an empty colon range)
        return float(y.mean()), 0.0
    bins = temp[0] + dbin * np.arange(int(np.floor((temp[-1] - temp[0]) / dbin + 1e-10)) + 1)   # :20
    nums = hist_centres(y, bins)                                           # :21
    b, sn, _ = fit_gauss1(bins, nums, 0.3, 3)                              # :29
    if b < bmin:                                                           # :31-34
        b = bmin
        sn = fit_gauss1(bins - bmin, nums, 0.3, 3, True)[1]
    return b, sn


def remove_baseline(y, sn):
    """[y, b] = remove_baseline(y, sn) (remove_baseline.m:6-10)"""
    y = np.asarray(y, dtype=np.float64).ravel()
    y_diff = np.r_[-1.0, np.diff(y)]
    sel = y[(y_diff >= 0) & (y_diff < sn)]
    b = np.median(sel) if sel.size else np.nan
    return y - b, b


def ordfilt2_max(v, n):
    """ordfilt2(v, n^2, true(n)): the maximum of the n x n neighbourhood, zeros outside the image, an even n centred at floor((n + 1) / 2)"""
    v = np.asarray(v, dtype=np.float64)
    c0 = (n + 1) // 2 - 1
    vp = np.pad(v, ((c0, n - 1 - c0), (c0, n - 1 - c0)))
    out = np.full(v.shape, -np.inf)
    for i in range(n):
        for j in range(n):
            np.maximum(out, vp[i:i + v.shape[0], j:j + v.shape[1]], out=out)
    return out


def connectivity_constraint(img, thr=0.01, sz=5):
    """img = connectivity_constraint(img) (connectivity_constraint.m:12-18) of one small image: open with a sz x sz square, threshold at thr * max(img), keep
    the 4-connected component that holds the maximum of img"""
    img = np.array(img, dtype=np.float64)
    ind_max = int(np.argmax(img.reshape(-1, order="F")))
    er = ndi.minimum_filter(img, size=sz, mode="constant", cval=np.inf)
    ai_open = ndi.maximum_filter(er, size=sz, mode="constant", cval=-np.inf)
    lab, _ = ndi.label(ai_open > img.max() * thr, structure=CROSS4)
    img[lab != lab[ind_max % img.shape[0], ind_max // img.shape[0]]] = 0
    return img


def imfilter_replicate(img, psf):
    """imfilter(img, psf, 'replicate') of one image: correlation about the origin floor((n + 1) / 2) of the kernel"""
    img = np.asarray(img, dtype=np.float64); psf = np.asarray(psf, dtype=np.float64)
    n0, n1 = psf.shape
    cr, cc = (n0 + 1) // 2 - 1, (n1 + 1) // 2 - 1
    ip = np.pad(img, ((cr, n0 - 1 - cr), (cc, n1 - 1 - cc)), mode="edge")
    out = np.zeros_like(img)
    for i, j in zip(*np.nonzero(psf)):
        out += psf[i, j] * ip[i:i + img.shape[0], j:j + img.shape[1]]
    return out


def refine_ac(ai_img, ci, sn_ci, connected=True, min_pixels=5):
    """extract_ac.m:60-107 after the regression: (ai image, ci, success).  sn_ci = GetSn(ci) (:89)."""
    ai = circular_constraints(ai_img)                                      # :61
    if connected:
        ai = connectivity_constraint(ai)                                   # :64-66
    if np.count_nonzero(ai > 0) < min_pixels:                              # :75-78
        return ai, ci, False
    b, sn = estimate_baseline_noise(ci)                                    # :88
    if sn > sn_ci:                                                         # :90-95
        ci = remove_baseline(ci, sn_ci)[0]
    else:
        ci = ci - b
    return ai, ci, bool(np.linalg.norm(ai) != 0)                           # :103-107


# --------------------------------------------------------------------------------------
# imresize along one dimension (options.ssub / options.tsub: greedyROI_endoscope.m:464-487, correlation_pnr_parallel.m:97-100, utilities/dsData.m:35)
# --------------------------------------------------------------------------------------
def _cubic_kernel(x):
    ax = np.abs(x); ax2 = ax * ax; ax3 = ax2 * ax
    return (1.5 * ax3 - 2.5 * ax2 + 1) * (ax <= 1) + (-0.5 * ax3 + 2.5 * ax2 - 4 * ax + 2) * ((ax > 1) & (ax <= 2))


def _box_kernel(x):
    return ((x >= -0.5) & (x < 0.5)).astype(np.float64)


def imresize_matrix(n_in, n_out, method="bicubic"):
    """The (n_out x n_in) float64 weight matrix of imresize(., [.. n_out ..], method) along one dimension of length n_in (the toolbox's documented
    `contributions` rule): scale = n_out / n_in, output sample x sits at u = x / scale + (1 - 1 / scale) / 2, the kernel ('box': -0.5 <= x < 0.5, 'bicubic':
    Keys, a = -0.5) is stretched by 1 / scale when shrinking (antialiasing is on), taps are mirrored at the border and every row is normalised to sum 1."""
    kernel, kw = {"box": (_box_kernel, 1.0), "bicubic": (_cubic_kernel, 4.0)}[method]
    n_in, n_out = int(n_in), int(n_out)
    scale = n_out / n_in
    if scale < 1:
        h = lambda x: scale * kernel(scale * x)
        kw = kw / scale
    else:
        h = kernel
    x = np.arange(1, n_out + 1, dtype=np.float64)
    u = x / scale + 0.5 * (1 - 1 / scale)
    left = np.floor(u - kw / 2)
    ind = left[:, None] + np.arange(int(np.ceil(kw)) + 2)[None, :]
    w = h(u[:, None] - ind)
    w = w / w.sum(axis=1, keepdims=True)
    aux = np.concatenate([np.arange(n_in), np.arange(n_in - 1, -1, -1)])   # [1:n n:-1:1], 0-based
    src = aux[np.mod(ind.astype(np.int64) - 1, aux.size)]
    M = np.zeros((n_out, n_in))
    np.add.at(M, (np.repeat(np.arange(n_out), src.shape[1]), src.ravel()), w.ravel())
    return M


def imresize_to(img, out_size, method="bicubic"):
    """imresize(img, [nr nc], method) on the first two dimensions of a float64 array (rows, then columns)"""
    img = np.asarray(img, dtype=np.float64)
    out = np.tensordot(imresize_matrix(img.shape[0], out_size[0], method), img, axes=(1, 0))
    return np.moveaxis(np.tensordot(imresize_matrix(img.shape[1], out_size[1], method), out, axes=(1, 1)), 0, 1)


def box_of(nr, nc, r, c, reach):
    """0-based half-open (r0, r1, c0, c1) of rsub x csub (greedyROI_endoscope.m:299-300,310-311) around the 0-based pixel (r, c)"""
    return max(0, r - reach), min(nr, r + reach + 1), max(0, c - reach), min(nc, c + reach + 1)


def greedy_roi_block(sess, Cn, PNR, gSiz, psf, min_corr, min_pnr, min_pixel, bd, K=None, connected=True, deconv=None, seeds=None, sig=3.0, on_step=None):
    """[results, center] = greedyROI_endoscope(Y, K, options) (greedyROI_endoscope.m:62-164,193-216,262-311,339-410,447-463) on one block, the video behind
    `sess`: sess.extract(r, c) -> (corr, ai, ci, stats) and sess.apply(r, c, ai, Hai, ci, sig, min_pnr, min_corr) -> (PNR, Cn) of the (4 gSiz + 1)^2 box,
    0-based block pixels (Engine.peel_extract / peel_apply).  Cn, PNR: the block's seed images.  bd = the four margins [top, bottom, left, right].
    deconv(ci_raw) -> (ci, ci_raw - b, si, pars) or None.  seeds: 0-based block pixels tried once, in the given order, under the halved thresholds of
    seed_method = 'manual' (:66-69); None = the automatic search.  on_step(kind, data): observer of every extract / apply (tests).
    Returns dict(A = list of ((r0, r1, c0, c1), ai image), C, C_raw, S, kernel_pars, center (k x 2, 1-based block coordinates))."""
    gSiz = int(gSiz)
    Cn = np.array(Cn, dtype=np.float64); PNR = np.array(PNR, dtype=np.float64)
    d1, d2 = Cn.shape
    min_v_search = min_corr * min_pnr                                      # :64
    if seeds is not None:                                                  # :66-69
        min_corr, min_pnr = min_corr / 2.0, min_pnr / 2.0
    with np.errstate(invalid="ignore"):
        PNR[PNR < min_pnr] = 0                                             # :135
        Cn[np.isnan(Cn)] = 0                                               # :147
        v_search = Cn * PNR                                                # :151
        v_search[(Cn < min_corr) | (PNR < min_pnr)] = 0                    # :152
    v_search[~np.isfinite(v_search)] = 0                                   # (a constant pixel, Sn = 0: never a seed; the reference leaves a NaN to medfilt2)
    ind_search = v_search == 0                                             # :153-154
    ind_bd = np.zeros((d1, d2), dtype=bool)                                # :160-164
    bd = [int(b) for b in bd]
    ind_bd[:bd[0], :] = True
    if bd[1] > 0: ind_bd[d1 - bd[1]:, :] = True
    ind_bd[:, :bd[2]] = True
    if bd[3] > 0: ind_bd[:, d2 - bd[3]:] = True
    nseed = int(np.count_nonzero(v_search > 0)) // 10                      # :194-198
    K = nseed if K is None else min(nseed, int(K))
    jj, ii = np.mgrid[1:d1 + 1, 1:d2 + 1]
    pixel_v = (ii * 10 + jj) * 1e-10                                       # :209-210
    tmp_d = max(3, int(np.floor(gSiz / 4.0 + 0.5)))                        # :215
    out_A, out_C, out_Craw, out_S, out_kp, center = [], [], [], [], [], []
    k = 0
    searching = True
    while searching and K > 0:
        v_search = medfilt2(v_search) + pixel_v                            # :216
        v_search[ind_search] = 0                                           # :217
        v_max = ordfilt2_max(v_search, tmp_d)                              # :218
        v_search[ind_bd] = 0                                               # :220
        if seeds is not None:                                              # :243-260: the clicks; an invalid one ends the list
            loc = []
            for (r, c) in seeds:
                if not (0 <= r < d1 and 0 <= c < d2) or v_search[r, c] == 0:
                    break
                loc.append((int(r), int(c)))
            searching = False                                              # (one round: the given pixels are tried once, in the given order)
        else:
            ind_search[v_search < min_v_search] = True                     # :263
            vf, mf = v_search.reshape(-1, order="F"), v_max.reshape(-1, order="F")
            ind = np.nonzero((vf == mf) & (mf > 0))[0]                     # :264
            ind = ind[np.argsort(-vf[ind], kind="stable")]                 # :267-268
            loc = [(int(i % d1), int(i // d1)) for i in ind]
        if not loc:
            break
        for (r, c) in loc:                                                 # :272
            max_v = v_search[r, c]
            ind_search[r, c] = True                                        # :280
            if max_v < min_v_search:                                       # :281-283
                continue
            corr, ai0, ci_raw, st = sess.extract(r, c)
            if on_step is not None:
                on_step("extract", dict(r=r, c=c, corr=corr, ai=ai0, ci=ci_raw, stats=st))
            if st["max_diff"] < 3 * st["std_diff"]:                        # :293
                continue
            ok = st["n_lo"] > 0 and np.isfinite(st["norm_ci"]) and st["norm_ci"] != 0      # extract_ac.m:29-33; an empty background set: y_bg = NaN
            if ok:
                ai, ci_raw, ok = refine_ac(ai0, ci_raw, st["sn_ci"], connected)
            if ok and (np.isnan(ai).any() or np.isnan(ci_raw).any()):      # :346
                ok = False
            if ok and (ai.sum() <= min_pixel or np.count_nonzero(ai > 0) < min_pixel):     # :347,351
                ok = False
            if not ok:
                continue
            k += 1
            if deconv is not None:                                         # :355-364
                ci, ci_keep, si, pars = deconv(ci_raw)
            else:                                                          # :366-369
                ci, ci_keep, si, pars = ci_raw, ci_raw, None, None
            ci = np.asarray(ci, dtype=np.float64)
            r0, r1, c0, c1 = box_of(d1, d2, r, c, gSiz)
            s0, s1, t0, t1 = box_of(d1, d2, r, c, 2 * gSiz)
            out_A.append(((r0, r1, c0, c1), ai)); out_C.append(ci); out_Craw.append(np.asarray(ci_keep, dtype=np.float64)); out_S.append(si); out_kp.append(pars)
            center.append((r + 1, c + 1))                                  # :372
            ind_search[r0:r1, c0:c1] |= ai > ai.max() * 0.5                # :375
            big = np.zeros((s1 - s0, t1 - t0))
            big[r0 - s0:r1 - s0, c0 - t0:c1 - t0] = ai
            Hai = imfilter_replicate(big, psf) if psf is not None else big     # :380-384
            pnr2, cn2 = sess.apply(r, c, ai, Hai, ci, sig, min_pnr, min_corr)  # :378,385-401
            if on_step is not None:
                on_step("apply", dict(r=r, c=c, ai=ai, ci=ci, Hai=Hai, pnr=pnr2, cn=cn2))
            PNR[s0:s1, t0:t1] = pnr2; Cn[s0:s1, t0:t1] = cn2               # :394,402
            v_search[s0:s1, t0:t1] = Cn[s0:s1, t0:t1] * PNR[s0:s1, t0:t1]  # :405
            v_search[ind_bd] = 0; v_search[ind_search] = 0                 # :406-407
            if k == K:                                                     # :447-450
                searching = False
                break
    return dict(A=out_A, C=out_C, C_raw=out_Craw, S=out_S, kernel_pars=out_kp, center=np.asarray(center, dtype=np.int64).reshape(-1, 2))


# --------------------------------------------------------------------------------------
# merging: the K x K side of merge_high_corr / merge_neurons_dist_corr / merge_close_neighbors (float64; the K x T side is the engine's)
# --------------------------------------------------------------------------------------
def footprint_overlap(A):
    """temp = A ./ sqrt(sum(A.^2, 1));  A_overlap = temp' * temp  (merge_high_corr.m:52-54) as a dense K x K float64 matrix; an empty footprint gives
    NaN in its row and column (0 * Inf), which fails every >= like the reference's"""
    A = sp.csc_matrix(A).astype(np.float64)
    ss = np.asarray(A.multiply(A).sum(axis=0)).ravel()
    with np.errstate(divide="ignore"):
        inv = 1.0 / np.sqrt(ss)
    ok = ss > 0
    temp = A @ sp.diags(np.where(ok, inv, 0.0))
    out = np.asarray((temp.T @ temp).todense())
    out[~ok, :] = np.nan; out[:, ~ok] = np.nan
    return out


def neuron_centers(A, d1, d2, method="max"):
    """(yy, xx), 1-based like the reference: [~, temp] = max(A, [], 1); [yy, xx] = ind2sub([d1 d2], temp)  (merge_neurons_dist_corr.m:64-65), or with
    method 'mean' / 'center' the centre of mass com(A, d1, d2) (utilities/com.m:20-28, clamped as :26-28).  Footprints are non-negative: a column without a positive
    entry reports pixel 1 as MATLAB's max of an all-zero column does."""
    A = sp.csc_matrix(A)
    K = A.shape[1]
    if str(method).lower() in ("mean", "center"):
        Af = A.astype(np.float64)
        pix = np.arange(d1 * d2)
        xy = np.vstack([pix % d1 + 1.0, pix // d1 + 1.0])
        with np.errstate(divide="ignore", invalid="ignore"):
            cm = (Af.T @ xy.T) / np.asarray(Af.sum(axis=0)).ravel()[:, None]
        cm = np.asarray(cm)
        cm[cm < 0] = 0
        cm[cm[:, 0] > d1, 0] = d1; cm[cm[:, 1] > d2, 1] = d2
        return cm[:, 0], cm[:, 1]
    ind = np.zeros(K, dtype=np.int64)
    for k in range(K):
        lo, hi = A.indptr[k], A.indptr[k + 1]
        if hi > lo:
            j = int(np.argmax(A.data[lo:hi]))             # (first maximum, rows ascending: MATLAB's tie rule)
            if A.data[lo + j] > 0:
                ind[k] = A.indices[lo + j]
    return (ind % d1 + 1).astype(np.float64), (ind // d1 + 1).astype(np.float64)


def center_distances(yy, xx):
    """dist_v = sqrt((xx - xx').^2 + (yy - yy').^2)  (merge_neurons_dist_corr.m:67)"""
    yy = np.asarray(yy, dtype=np.float64); xx = np.asarray(xx, dtype=np.float64)
    return np.sqrt((xx[:, None] - xx[None, :]) ** 2 + (yy[:, None] - yy[None, :]) ** 2)


def decay_times(kernel_pars):
    """taud(m) = ar2exp(kernel_pars(m))(1) for AR(1) (OASIS_matlab/functions/ar2exp.m:3-10): the roots of x^2 - g x are {g, 0}, d = max, tau_d = -1 / log(d)"""
    g = np.asarray(kernel_pars, dtype=np.float64).ravel()
    with np.errstate(divide="ignore", invalid="ignore"):
        return -1.0 / np.log(np.maximum(g, 0.0))


def merge_groups(flag):
    """graph_connected_comp(sparse(flag_merge)) with the singletons dropped (merge_high_corr.m:82-85): a list of ascending index arrays, ordered by their
    lowest member (the component labels of the reference follow the first node of each component)"""
    from scipy.sparse.csgraph import connected_components
    flag = np.asarray(flag, dtype=bool)
    K = flag.shape[0]
    if K == 0:
        return []
    n, lab = connected_components(sp.csr_matrix(flag | flag.T), directed=False)
    groups = [np.flatnonzero(lab == c) for c in range(n)]
    groups = [g for g in groups if g.size > 1]
    return sorted(groups, key=lambda g: int(g[0]))


def merge_iterate(G, M, niter=10):
    """The ten alternations ai = data ci' / (ci ci'), ci = ai' data / (ai' ai) of merge_high_corr.m:176-181 with data = A(:, IDs) C_raw(IDs, :) never formed:
    every ci lies in the row span of C_raw(IDs, :), ci = w' C_raw(IDs, :), and every ai in the column span of A(:, IDs), ai = A(:, IDs) g.  With
    G = C_raw(IDs, :) C_raw(IDs, :)' and M = A(:, IDs)' A(:, IDs) (n x n) the steps are g = G w / (w' G w), w = M g / (g' M g), starting from w = e1
    (ci = C_raw(IDs(1), :)).  Returns (g, w) after `niter` rounds."""
    G = np.asarray(G, dtype=np.float64); M = np.asarray(M, dtype=np.float64)
    w = np.zeros(G.shape[0]); w[0] = 1.0
    g = w
    for _ in range(niter):
        Gw = G @ w
        g = Gw / (w @ Gw)
        Mg = M @ g
        w = Mg / (g @ Mg)
    return g, w


# --------------------------------------------------------------------------------------
# The closing calls of demo_large_data_1p.m: orderROIs (Sources2D.m:573-653) and show_demixed_video (@Sources2D/show_demixed_video.m).  What is K x T or d x T runs
# on the engine (merge.hpp: k_trace_order_stats, demix.hpp: k_demix_panels); the sort, the display ranges and the montage are the host's.
# --------------------------------------------------------------------------------------
def matlab_sort_order(x, descend=False):
    """[~, srt] = sort(x) / sort(x, 'descend'), 0-based: MATLAB's sort is stable -- ties keep their order --, 'ascend' puts NaN last and 'descend' puts NaN first
    (among themselves the NaNs keep their order too).  The one statement of that rule."""
    x = np.asarray(x, dtype=np.float64).ravel()
    nan = np.flatnonzero(np.isnan(x))
    rest = np.flatnonzero(~np.isnan(x))
    if descend:
        return np.concatenate([nan, rest[np.argsort(-x[rest], kind="stable")]]).astype(np.int64)
    return np.concatenate([rest[np.argsort(x[rest], kind="stable")], nan]).astype(np.int64)


def matlab_uint16(x):
    """uint16(x) of a double array: round half away from zero, saturate to [0, 65535], NaN -> 0"""
    x = np.asarray(x, dtype=np.float64)
    r = np.where(np.isnan(x), 0.0, np.sign(x) * np.floor(np.abs(x) + 0.5))
    return np.clip(r, 0.0, 65535.0).astype(np.uint16)


def prism64():
    """prism(64): MATLAB's prism colormap repeats red, orange, yellow, green, blue, violet"""
    six = np.array([[1.0, 0.0, 0.0], [1.0, 0.5, 0.0], [1.0, 1.0, 0.0], [0.0, 1.0, 0.0], [0.0, 0.0, 1.0], [2.0 / 3.0, 0.0, 1.0]])
    return six[np.arange(64) % 6]


def demix_ranges(amp_ac, raw_samples=None, range_ac=None, range_Y=None, multi_factor=None):
    """the display ranges of show_demixed_video.m:39-57 as a dict (range_ac, range_res, range_Y, multi_factor).  raw_samples: the values the default range_Y is
    taken from (quantiles 0.01 and 0.98; with a given multi_factor the 0.01 quantile alone) -- needed only when range_Y is None"""
    amp_ac = float(amp_ac)
    range_ac = amp_ac * np.array([0.01, 1.01]) if range_ac is None else np.asarray(range_ac, dtype=np.float64).ravel()      # :39-41
    range_res = range_ac - range_ac.mean()                                                                                    # :42
    given_mf = multi_factor is not None
    if range_Y is None:                                                                                                       # :43-52
        if raw_samples is None:
            raise ValueError("demix_ranges: the default range_Y needs samples of the raw video")
        if not given_mf:
            temp = matlab_quantile(raw_samples, [0.01, 0.98])
            multi_factor = float(np.ceil((temp[1] - temp[0]) / (range_ac[1] - range_ac[0])))
        else:
            temp = matlab_quantile(raw_samples, [0.01])
        center_Y = temp[0] + multi_factor * amp_ac / 2
        range_Y = center_Y + range_res * multi_factor
    else:
        range_Y = np.asarray(range_Y, dtype=np.float64).ravel()
    if not given_mf and multi_factor is None:                                                                                 # :54-57 (a given range_Y)
        multi_factor = float(np.round((range_Y[1] - range_Y[0]) / (range_ac[1] - range_ac[0])))
        range_Y = (range_res - range_res[0]) * multi_factor + range_Y[0]
    return dict(range_ac=range_ac, range_res=range_res, range_Y=np.asarray(range_Y, dtype=np.float64), multi_factor=float(multi_factor))


def imagesc_8bit(v, lo, hi):
    """imagesc(v, [lo hi]) through a 256-entry grey map: floor(256 (v - lo) / (hi - lo)) clipped to 0 .. 255 (NaN -> 0)"""
    with np.errstate(invalid="ignore", divide="ignore"):
        q = np.floor(256.0 * (np.asarray(v, dtype=np.float64) - lo) / (hi - lo))
    return np.clip(np.nan_to_num(q, nan=0.0, posinf=255.0, neginf=0.0), 0, 255).astype(np.uint8)


def demixed_montage(frame, ranges):
    """one displayed frame as a (2 d1) x (3 d2) x 3 uint8 image in the positions of show_demixed_video.m:83-88 -- top: raw, raw - background, residual; bottom:
    background, denoised, demixed.  frame: dict of d1 x d2 panels (mixed: d1 x d2 x 3 uint16, shown as truecolor: its high byte); no titles, no time stamp"""
    rY, rac, rres = ranges["range_Y"], ranges["range_ac"], ranges["range_res"]
    grey = lambda v, r: np.repeat(imagesc_8bit(v, r[0], r[1])[:, :, None], 3, axis=2)
    top = np.concatenate([grey(frame["raw"], rY), grey(frame["signal"], rac), grey(frame["residual"], rres)], axis=1)
    bottom = np.concatenate([grey(frame["bg"], rY), grey(frame["denoised"], rac), (np.asarray(frame["mixed"], dtype=np.uint16) >> 8).astype(np.uint8)], axis=1)
    return np.concatenate([top, bottom], axis=0)
