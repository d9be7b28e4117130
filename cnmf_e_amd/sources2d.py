"""Host-side mirror of the reference's ``Sources2D`` update methods on top of the HIP engine.

The reference is MATLAB (`ca_source_extraction/@Sources2D/`); there is no MATLAB in the build image,
so the host side above the C ABI is Python and keeps the reference's names, argument meaning and
error behaviour for the ONE path this project covers:

    update_background_parallel(use_parallel)            @Sources2D/update_background_parallel.m:1
    update_spatial_parallel(use_parallel, update_sn)    @Sources2D/update_spatial_parallel.m:1
    update_temporal_parallel(use_parallel, use_c_hat)   @Sources2D/update_temporal_parallel.m:1

Per-patch slicing (which neurons / pixels go to which patch, how results are stitched) is host
logic exactly as in the reference; every numerical kernel runs on the GPU through
``cnmf_e_amd.engine.Engine`` (no CPU fallback).  Patches can be sharded over ranks of a
``torch.distributed`` group (one process per GPU): background and spatial updates need no
collective on the data path, the temporal update does ONE all-reduce of ``aa .* C_raw`` and ``aa``
(update_temporal_parallel.m:269-280).
"""
from __future__ import annotations

from dataclasses import dataclass, field
from typing import Optional

import ctypes
import os

import numpy as np
import scipy.sparse as sp

from . import _lib as L
from . import hostops
from .engine import BoundRows, DeviceTraces, Engine

__all__ = ["Options", "PatchedVideo", "Sources2D", "distribute_geometry", "determine_search_location", "seed_psf", "bspline_basis"]


# --------------------------------------------------------------------------------------
# options actually read by the hot path (CNMFSetParms.m)
# --------------------------------------------------------------------------------------
@dataclass
class Options:
    d1: int = 0
    d2: int = 0
    ring_radius: int = 15            # CNMFSetParms.m:106
    num_neighbors: int | None = None  # :109
    bg_ssub: int = 1                 # :107
    bg_acceleration: bool = True     # :108
    thresh_outlier: float = float("nan")   # :112
    background_model: str = "ring"   # demo_large_data_1p.m:54
    spatial_algorithm: str = "hals"  # :117  ('hals' | 'hals_thresh' | 'nnls')
    search_method: str = "ellipse"   # :48
    se: object = "disk4"             # strel('disk', 4, 0): element of the 'dilate' search; None = [] -> strel('disk', bSiz, 0)
    bSiz: int = 3                    # :35
    nb: int = 1                      # :23 (threshold_components leaves the last nb columns alone)
    nrgthr: float = 0.99             # :56
    min_size: float = 3.0            # :51
    max_size: float = 8.0            # :52
    dist: float = 3.0                # :53
    maxIter: int = 5                 # :36
    deconv_flag: bool = False        # :101
    deconv_options: dict = field(default_factory=lambda: {"type": "ar1", "method": "foopsi", "smin": -5.0,
                                                          "optimize_pars": True, "optimize_b": True, "max_tau": 100.0})   # demo_large_data_1p.m:38-43
    spatial_constraints: dict = field(default_factory=lambda: {"circular": False, "connected": True})   # :116
    # the seed images (correlation_pnr_parallel): demo_large_data_1p.m:16-17,45-47,76 and the reference's defaults for the rest
    gSig: float = 3.0                # width of the Gaussian kernel that approximates one neuron; <= 0: no spatial filter
    gSiz: float = 13.0               # neuron diameter
    center_psf: bool = True          # subtract the kernel's mean over its support (1p data)
    nk: int = 1                      # knots of the detrending spline basis; 1 = no detrending
    detrend_method: str = "spline"   # 'spline' | 'local_min' (only 'spline' is built)
    ssub: int = 1                    # spatial / temporal down-sampling of the seed images and the first initialisation (dsData.m): ssub in 1..8, tsub >= 1;
    tsub: int = 1                    # both are read where Sources2D is constructed (Sources2D._ds_factors)
    # the greedy initialisation (initComponents_parallel): CNMFSetParms.m names at :19,97-100, their defaults at :209,286-289
    min_corr: float = 0.3            # :19 / :209   minimum local correlation of a seed pixel
    min_pnr: float = 10.0            # :97 / :286   minimum peak-to-noise ratio of a seed pixel
    seed_method: str = "auto"        # :98 / :287   'auto' | 'manual' (manual = the `seeds` argument of initComponents_parallel)
    min_pixel: float = 5.0           # :99 / :288   minimum number of non-zero pixels of a neuron
    bd: int | None = 3               # :100 / :289  margin of the FOV without seed pixels; None = [] -> gSiz (initComponents_parallel.m:200-203)
    K: int | None = None             # maximum number of neurons per patch (initComponents_parallel's argument; None = [] -> as many as are found)
    # merging (merge_high_corr, merge_neurons_dist_corr, merge_close_neighbors): CNMFSetParms.m names at :70,110-111, their defaults at :260,299-300
    merge_thr: object = 0.85         # :70 / :260   scalar, or [A overlap, corr(C), corr(S)] (+ a fourth entry: the largest difference of the decay times)
    dmin: object = 1.0               # :110 / :299  largest distance of two neuron centres that may merge (merge_close_neighbors: + a second entry, decay times)
    method_dist: str = "max"         # :111 / :300  'max' (the footprint's brightest pixel) | 'mean' / 'center' (its centre of mass)
    # dF/F (extract_DF_F_endoscope): CNMFSetParms.m:73-74
    df_prctile: float = 50           # :73   percentile of the projected background that is the baseline
    df_window: Optional[int] = None  # :74   length of the running window in frames; None = [] (or longer than the recording): one baseline per neuron


def _mround(x):
    return np.sign(x) * np.floor(np.abs(x) + 0.5)


def distribute_geometry(d1, d2, patch_dims, w_overlap):
    """patch_pos / block_pos exactly as endoscope/distribute_data.m:38-100,161-173 lays them out
    (1-based inclusive [r0 r1 c0 c1]; block = patch grown by w_overlap+1, clipped)."""
    minw = 2 * w_overlap + 3
    pd = np.atleast_1d(np.asarray(patch_dims, dtype=np.float64)).copy()
    pd[pd < minw] = minw
    pd = np.array([pd[0], pd[0]]) if pd.size == 1 else pd[:2]
    nrp, ncp = int(_mround(d1 / pd[0])), int(_mround(d2 / pd[1]))

    def edges(n, dd, rows):
        if n <= 1:
            return np.array([1, dd], dtype=np.int64)
        e = np.ceil(np.linspace(1, dd, n + 1)).astype(np.int64)
        if rows:
            e[-1] = dd
        if e[1] - e[0] < minw:
            e = np.arange(1, dd + 1, minw, dtype=np.int64)
            e[-1] = dd
        return e

    er, ec = edges(nrp, d1, True), edges(ncp, d2, False)
    nrp, ncp = er.size - 1, ec.size - 1
    patch_pos, block_pos = {}, {}
    for m in range(nrp):
        for n in range(ncp):
            patch_pos[(m, n)] = np.array([er[m], er[m + 1] - (m != nrp - 1), ec[n], ec[n + 1] - (n != ncp - 1)], dtype=np.int64)
            block_pos[(m, n)] = np.array([max(1, er[m] - w_overlap - 1), min(d1, er[m + 1] + w_overlap),
                                          max(1, ec[n] - w_overlap - 1), min(d2, ec[n + 1] + w_overlap)], dtype=np.int64)
    return (nrp, ncp), patch_pos, block_pos


def nearest_rows(n, s):
    """0-based input rows that imresize(., 1/s, 'nearest') keeps along a dimension of length n (box kernel on u = x*s + 0.5*(1 - s), taps
    mirrored at the border; the same selection the engine's cnmfe_patch_derive makes): ceil(n/s) of them"""
    x = np.arange(1, -(-n // s) + 1, dtype=np.float64)
    ind = np.floor(x * s + 0.5 * (1 - s) + 0.5).astype(np.int64)          # 1-based
    ind = np.where(ind > n, 2 * n + 1 - ind, ind)
    return ind - 1


def storage_block_index(d, patch_idx, w_overlap):
    """block_idx_r / block_idx_c of distribute_data.m:91-97: the cut lines of the blocks the reference stores the video in"""
    idx = np.concatenate([np.asarray(patch_idx) - 1 - w_overlap, np.asarray(patch_idx) + w_overlap])
    return np.unique(np.clip(idx, 1, d))


def estimate_noise_image(sn_pix, block_idx_r, block_idx_c):
    """Sources2D.m:361-376 given the per-pixel estimates: the reference evaluates storage block [r0 r1] x [c0 c1] INCLUDING the row r1 it
    shares with the next block, then drops row END-1 (not the shared one) of every block but the last, likewise for columns.  Net effect:
    row b - 1 of the image holds the estimate of row b for every interior cut line b -- reproduced as it is."""
    out = np.array(sn_pix, copy=True)
    for b in np.asarray(block_idx_r)[1:-1]:
        out[b - 2, :] = out[b - 1, :]
    for b in np.asarray(block_idx_c)[1:-1]:
        out[:, b - 2] = out[:, b - 1]
    return out


def _fspecial_gaussian(n, sigma):
    """fspecial('gaussian', n, sigma) (MathWorks documentation): exp(-(x^2 + y^2) / (2 sigma^2)) on the n x n grid centred on 0, entries below eps * max
    zeroed, normalised to sum 1"""
    x = np.arange(n, dtype=np.float64) - (n - 1) / 2.0
    h = np.exp(-(x[:, None] ** 2 + x[None, :] ** 2) / (2.0 * sigma * sigma))
    h[h < np.finfo(np.float64).eps * h.max()] = 0.0
    return h / h.sum()


def seed_psf(gSig, gSiz, center_psf=True):
    """The spatial filter of the seed images (correlation_image_endoscope.m:36-47), float64, odd-sized; None for gSig <= 0 (no filter).
    center_psf: the Gaussian of ceil(4 gSig + 1) pixels, its mean over the support {psf >= max of its first column} subtracted, 0 outside the support.
    Otherwise the plain Gaussian of round(gSiz) pixels; an even-sized one gets a leading zero row and column, which keeps imfilter's origin
    floor((n + 1) / 2) of the even kernel at the centre of the odd one (the engine filters with odd kernels only)."""
    if gSig <= 0:
        return None
    if center_psf:
        psf = _fspecial_gaussian(int(np.ceil(gSig * 4 + 1)), gSig)
        ind = psf >= psf[:, 0].max()
        psf = psf - psf[ind].mean()
        psf[~ind] = 0.0
        n = psf.shape[0]
    else:
        n = int(_mround(gSiz))
        psf = _fspecial_gaussian(n, gSig)
    if n % 2 == 0:
        pad = np.zeros((n + 1, n + 1))
        pad[1:, 1:] = psf
        psf = pad
    return psf


def bspline_basis(T, nk, order=4):
    """X = bsplineM((1:T)', linspace(1, T, nk), 4) of detrend_data.m:23: the nk + order - 2 B-splines of that order on the breaks with order-fold end knots,
    evaluated at the frames 1..T (T x (nk + order - 2), float64; rows sum to 1).  Plain de Boor recursion over the knot interval of every frame."""
    T, nk, k = int(T), int(nk), int(order)
    if nk < 2:
        raise ValueError("a spline basis needs at least 2 knots")
    x = np.arange(1, T + 1, dtype=np.float64)
    breaks = np.linspace(1.0, float(T), nk)
    knots = np.concatenate([np.full(k - 1, breaks[0]), breaks, np.full(k - 1, breaks[-1])])
    nbasis = knots.size - k
    # knots[left] <= x < knots[left + 1], the last frame in the last non-empty interval
    left = np.clip(np.searchsorted(knots, x, side="right") - 1, k - 1, nbasis - 1)
    b = np.zeros((T, k))
    b[:, 0] = 1.0
    for j in range(1, k):
        saved = np.zeros(T)
        for r in range(j):
            tr = knots[left + r + 1] - x
            tl = x - knots[left + r + 1 - j]
            term = b[:, r] / (tr + tl)
            b[:, r] = saved + tr * term
            saved = tl * term
        b[:, j] = saved
    X = np.zeros((T, nbasis))
    rows = np.arange(T)
    for r in range(k):
        X[rows, left - (k - 1) + r] = b[:, r]
    return X


def _rect_pixels(rect, d1):
    """global column-major pixel indices of a rectangle, in the rectangle's own column-major order"""
    r0, r1, c0, c1 = [int(v) for v in rect]
    rr = np.arange(r0 - 1, r1)
    cc = np.arange(c0 - 1, c1)
    return (cc[None, :] * d1 + rr[:, None]).reshape(-1, order="F")


def determine_search_location(A, d1, d2, min_size=3.0, max_size=8.0, dist=3.0, native=True):
    """'ellipse' search masks, utilities/determine_search_location.m:50-104 + utilities/com.m:20-28.
    Vectorised over neurons; returns a boolean CSC matrix (d x K)."""
    d, K = A.shape
    mom = _footprint_moments_native(A, d1, d2) if native and K > 0 and d < 2 ** 31 else None
    if mom is not None:
        empty, cmx, cmy, vxx, vxy, vyy = mom
    else:
        A = sp.csc_matrix(A, dtype=np.float64)
        A.sort_indices()
        coo = A.tocoo()
        pix, col, val = coo.row, coo.col, coo.data
        x = (pix % d1 + 1).astype(np.float64)
        y = (pix // d1 + 1).astype(np.float64)
        s = np.bincount(col, weights=val, minlength=K)
        empty = s == 0                                                        # :52
        ss = np.where(empty, 1.0, s)
        cmx = np.bincount(col, weights=val * x, minlength=K) / ss             # com.m:24
        cmy = np.bincount(col, weights=val * y, minlength=K) / ss
        cmx = np.clip(cmx, 0, d1); cmy = np.clip(cmy, 0, d2)                  # com.m:26-28
        dx, dy = x - cmx[col], y - cmy[col]
        vxx = np.bincount(col, weights=val * dx * dx, minlength=K) / ss       # :73
        vxy = np.bincount(col, weights=val * dx * dy, minlength=K) / ss
        vyy = np.bincount(col, weights=val * dy * dy, minlength=K) / ss
    M = np.stack([np.stack([vxx, vxy], -1), np.stack([vxy, vyy], -1)], -2)
    D, V = np.linalg.eigh(M)                                              # :74 ascending eigenvalues
    d11 = np.minimum(max_size ** 2, np.maximum(min_size ** 2, D[:, 0]))   # :81
    d22 = np.minimum(max_size ** 2, np.maximum(min_size ** 2, D[:, 1]))   # :82
    # candidate window: the ellipse reaches dist*sqrt(d22) from the centre along its long axis (d22 <= max_size^2); sizing the window by the
    # largest ellipse actually present instead of the largest possible one cuts the (K, W, W) arrays below ~3x for typical footprints
    R = min(int(np.ceil(dist * max_size)), int(np.ceil(dist * np.sqrt(float(d22.max()) if K else 0.0)))) + 1
    if native and K > 0 and d < 2 ** 31:
        # the window test (:84) in the library's host helper: per image column the run of rows, its ends settled with the same expression in the same
        # order as below -- identical masks (tests/test_host_logic.py) in ~0.2 ms instead of 7-20 ms of (K, W, W) array passes, which had become the
        # host's critical path between the ring fit and the spatial update once the fit took under 9 ms
        try:
            fn = L.lib.cnmfe_search_ellipse
        except (ImportError, OSError, AttributeError):
            fn = None
        if fn is not None:
            vk = np.ascontiguousarray(np.stack([V[:, 0, 0], V[:, 1, 0], V[:, 0, 1], V[:, 1, 1]], -1), dtype=np.float64)
            cx = np.ascontiguousarray(cmx, dtype=np.float64); cy = np.ascontiguousarray(cmy, dtype=np.float64)
            a11 = np.ascontiguousarray(d11, dtype=np.float64); a22 = np.ascontiguousarray(d22, dtype=np.float64)
            em = np.ascontiguousarray(empty, dtype=np.uint8)
            optr = np.empty(K + 1, dtype=np.int64); nn = np.zeros(1, dtype=np.int64)
            cap = int(K) * (2 * R + 1) ** 2
            orow = np.empty(max(cap, 1), dtype=np.int32)
            rc = fn(int(K), int(d1), int(d2), cx.ctypes.data, cy.ctypes.data, vk.ctypes.data, a11.ctypes.data, a22.ctypes.data, em.ctypes.data, float(dist), int(R),
                    cap, optr.ctypes.data, orow.ctypes.data, nn.ctypes.data)
            if rc != 0:
                raise ValueError(L.lib.cnmfe_last_error().decode())
            n = int(nn[0])
            IND = sp.csc_matrix((np.ones(n, dtype=bool), orow[:n].copy(), optr), shape=(d, K))
            IND.has_sorted_indices = True
            return IND
    off = np.arange(-R, R + 1)
    rows = np.floor(cmx)[:, None] + off[None, :]                           # (K, W) candidate rows (1-based)
    cols = np.floor(cmy)[:, None] + off[None, :]
    ex = rows - cmx[:, None]
    ey = cols - cmy[:, None]
    # (cor*V(:,1))^2/d11 + (cor*V(:,2))^2/d22 <= dist^2                    (:84)
    p1 = ex[:, :, None] * V[:, 0, 0][:, None, None] + ey[:, None, :] * V[:, 1, 0][:, None, None]
    p2 = ex[:, :, None] * V[:, 0, 1][:, None, None] + ey[:, None, :] * V[:, 1, 1][:, None, None]
    inside = np.sqrt(p1 ** 2 / d11[:, None, None] + p2 ** 2 / d22[:, None, None]) <= dist
    inside &= (rows >= 1)[:, :, None] & (rows <= d1)[:, :, None] & (cols >= 1)[:, None, :] & (cols <= d2)[:, None, :]
    inside &= ~empty[:, None, None]                                        # :102-104
    kk, ri, ci = np.nonzero(inside)
    gp = ((cols[kk, ci] - 1) * d1 + (rows[kk, ri] - 1)).astype(np.int64)
    IND = sp.csc_matrix((np.ones(kk.size, dtype=bool), (gp, kk)), shape=(d, K))
    IND.sort_indices()
    return IND


def _footprint_moments_native(A, d1, d2):
    """(empty, cmx, cmy, vxx, vxy, vyy) of determine_search_location by the library's host helper cnmfe_footprint_moments (the same sums in the same order as the
    bincount formulation, in one pass over A); None when the library is not built or A is not a sorted float32 / int32 CSC matrix"""
    if not sp.isspmatrix_csc(A) or A.data.dtype != np.float32 or A.indices.dtype != np.int32 or not A.has_sorted_indices:
        return None
    try:
        fn = L.lib.cnmfe_footprint_moments
    except (ImportError, OSError, AttributeError):
        return None
    K = A.shape[1]
    indptr = A.indptr if A.indptr.dtype == np.int64 else A.indptr.astype(np.int64)
    out = np.empty((6, K), dtype=np.float64); em = np.empty(K, dtype=np.uint8)
    rc = fn(int(K), int(d1), int(d2), indptr.ctypes.data, A.indices.ctypes.data, A.data.ctypes.data, out[0].ctypes.data, em.ctypes.data,
            out[1].ctypes.data, out[2].ctypes.data, out[3].ctypes.data, out[4].ctypes.data, out[5].ctypes.data)
    if rc != 0:
        raise ValueError(L.lib.cnmfe_last_error().decode())
    return em.astype(bool), out[1], out[2], out[3], out[4], out[5]


def rows_of(A, lut, nloc, cols=None, span=None, cand=None):
    """A(rows, :) for the rows a lookup table selects (global pixel -> local row or -1; local order ascending with the global one), as
    (ind, A(rows, ind)) in CSC with ind = the columns whose selected entries sum to > 0 (`sum(A(mask,:),1) > 0`, the reference's neuron
    selection) -- or, with `cols` (ascending) given, A(rows, cols).  No CSR conversion and no per-row index array: columns that cannot reach
    the rows (first / last stored row outside `span` = (lowest, highest) selected global row) are dropped in O(K), the rest costs O(their nnz)."""
    A = A if sp.isspmatrix_csc(A) else sp.csc_matrix(A)
    if not A.has_sorted_indices:
        A = A.copy(); A.sort_indices()
    K = A.shape[1]
    if cols is None and cand is not None:
        cand = np.asarray(cand, dtype=np.int64)                      # the caller's prefilter (a superset of the columns that can reach the rows)
    elif cols is None:
        cnt_all = np.diff(A.indptr)
        cand = np.nonzero(cnt_all > 0)[0]
        if span is not None and cand.size:
            first = A.indices[A.indptr[cand]]; last = A.indices[A.indptr[cand + 1] - 1]
            cand = cand[(last >= span[0]) & (first <= span[1])]
    else:
        cand = np.asarray(cols, dtype=np.int64)
        if cand.size and np.any(np.diff(cand) < 0):
            raise ValueError("cols must be ascending")
    M = _select_rows_native(A, lut, nloc, cand, cols is not None)
    if M is not None:
        return M
    return _select_rows_numpy(A, lut, nloc, cand, cols is not None)


def _csc_fast(data, indices, indptr, shape):
    """a scipy CSC matrix around arrays that ARE a valid CSC structure with ascending row indices inside every column (what the library's host helpers return):
    the constructor's format checks and the later has_sorted_indices scans cost 50-100 us per matrix, and a rank of a sharded run builds ~10 small ones per patch
    and iteration (scripts/host_python_profile.py: 3.1 ms of Python per iteration for two 128 x 128 patches, a third of it here)"""
    M = sp.csc_matrix.__new__(sp.csc_matrix)
    M._shape = (int(shape[0]), int(shape[1])); M.maxprint = 50
    if indptr.dtype != indices.dtype:                          # (scipy's kernels want one index type: the column pointers follow the row indices, as its constructor does)
        indptr = indptr.astype(indices.dtype)
    M.data, M.indices, M.indptr = data, indices, indptr
    M.has_sorted_indices = True
    return M


def _csc_from_triplets(r, c, v, shape):
    """the CSC matrix of DISJOINT (row, column, value) triplets (ValueError on a pair given twice): one counting pass in the library's host helper
    (cnmfe_csc_from_triplets) -- scipy's COO -> CSC conversion sorts the whole list, and every rank of a sharded run assembles the WHOLE gathered A; falls back
    to scipy without the library"""
    r = np.ascontiguousarray(r, dtype=np.int32); c = np.ascontiguousarray(c, dtype=np.int32); v = np.ascontiguousarray(v, dtype=np.float32)
    try:
        fn = L.lib.cnmfe_csc_from_triplets
    except (ImportError, OSError, AttributeError):                # (no library, or a CNMFE_LIB build without the helper)
        return sp.csc_matrix((v, (r, c)), shape=shape)
    n = int(r.size)
    optr = np.empty(shape[1] + 1, dtype=np.int64); orow = np.empty(max(n, 1), dtype=np.int32); oval = np.empty(max(n, 1), dtype=np.float32)
    rc = fn(n, r.ctypes.data, c.ctypes.data, v.ctypes.data, int(shape[1]), int(shape[0]), optr.ctypes.data, orow.ctypes.data, oval.ctypes.data)
    if rc != 0:
        # PRECONDITION: disjoint triplets (the patches' rows are, update_spatial_parallel.m:324-334).  A pair given twice -- which scipy's conversion would sum
        # silently -- or an index out of range is an error of the caller, reported as such
        raise ValueError(L.lib.cnmfe_last_error().decode())
    return _csc_fast(oval[:n], orow[:n], optr, shape)


def _select_rows_native(A, lut, nloc, cand, keep_all):
    """rows_of's selection by the library's host helper cnmfe_csc_select_rows (one pass over the candidates' entries in C: ~10x the NumPy
    formulation below at the 100-neuron patches of a 4 x 4 decomposition, where six such slices per patch and iteration were most of the
    host's time).  None when the library is not built (host-logic tests on a checkout without it) or the matrix is not int32 / float32."""
    if A.indices.dtype != np.int32 or A.data.dtype != np.float32 or lut.dtype != np.int32:
        return None
    try:
        fn = L.lib.cnmfe_csc_select_rows
    except (ImportError, OSError):
        return None
    indptr = A.indptr if A.indptr.dtype == np.int64 else A.indptr.astype(np.int64)
    cand = np.ascontiguousarray(cand, dtype=np.int64)
    nc = int(cand.size)
    cap = int((indptr[cand + 1] - indptr[cand]).sum()) if nc else 0
    ind = np.empty(nc, dtype=np.int64); optr = np.empty(nc + 1, dtype=np.int64)
    orow = np.empty(max(cap, 1), dtype=np.int32); oval = np.empty(max(cap, 1), dtype=np.float32)
    nk = ctypes.c_int64(0)
    rc = fn(indptr.ctypes.data, A.indices.ctypes.data, A.data.ctypes.data, lut.ctypes.data, nc, cand.ctypes.data, 1 if keep_all else 0, cap,
            ind.ctypes.data, optr.ctypes.data, orow.ctypes.data, oval.ctypes.data, ctypes.byref(nk))
    if rc != 0:
        raise ValueError(L.lib.cnmfe_last_error().decode())
    nk = nk.value
    n = int(optr[nk])
    return ind[:nk], _csc_fast(oval[:n], orow[:n], optr[:nk + 1], (nloc, nk))


def _select_block_patch_native(A, lut_b, nb, lut_p, npx, cand):
    """(ind, A(block, ind), A(patch, ind)) in ONE pass of the library's host helper cnmfe_csc_select_block_patch -- what two rows_of calls give (the temporal update asks
    for both per patch, update_temporal_parallel.m:83-91, on the spatial -> temporal hand-over where the device waits for the host); None when the helper cannot run"""
    if A.indices.dtype != np.int32 or A.data.dtype != np.float32 or lut_b.dtype != np.int32 or lut_p.dtype != np.int32:
        return None
    try:
        fn = L.lib.cnmfe_csc_select_block_patch
    except (ImportError, OSError, AttributeError):
        return None
    indptr = A.indptr if A.indptr.dtype == np.int64 else A.indptr.astype(np.int64)
    cand = np.ascontiguousarray(cand, dtype=np.int64)
    nc = int(cand.size)
    cap = int((indptr[cand + 1] - indptr[cand]).sum()) if nc else 0
    ind = np.empty(nc, dtype=np.int64); bptr = np.empty(nc + 1, dtype=np.int64); pptr = np.empty(nc + 1, dtype=np.int64)
    brow = np.empty(max(cap, 1), dtype=np.int32); bval = np.empty(max(cap, 1), dtype=np.float32)
    prow = np.empty(max(cap, 1), dtype=np.int32); pval = np.empty(max(cap, 1), dtype=np.float32)
    nk = ctypes.c_int64(0)
    rc = fn(indptr.ctypes.data, A.indices.ctypes.data, A.data.ctypes.data, lut_b.ctypes.data, lut_p.ctypes.data, nc, cand.ctypes.data, cap,
            ind.ctypes.data, bptr.ctypes.data, brow.ctypes.data, bval.ctypes.data, pptr.ctypes.data, prow.ctypes.data, pval.ctypes.data, ctypes.byref(nk))
    if rc != 0:
        raise ValueError(L.lib.cnmfe_last_error().decode())
    nk = nk.value
    n_b, n_p = int(bptr[nk]), int(pptr[nk])
    return ind[:nk], _csc_fast(bval[:n_b], brow[:n_b], bptr[:nk + 1], (nb, nk)), _csc_fast(pval[:n_p], prow[:n_p], pptr[:nk + 1], (npx, nk))


def _bbox_native(A, d1):
    """(non-empty columns, first / last image row, first / last image column) of a sorted int32 CSC footprint matrix by cnmfe_csc_bbox; None when the helper cannot run"""
    if A.indices.dtype != np.int32 or not A.has_sorted_indices:
        return None
    try:
        fn = L.lib.cnmfe_csc_bbox
    except (ImportError, OSError, AttributeError):
        return None
    K = A.shape[1]
    indptr = A.indptr if A.indptr.dtype == np.int64 else A.indptr.astype(np.int64)
    nz = np.empty(max(K, 1), dtype=np.int64); box = np.empty((4, max(K, 1)), dtype=np.int32)
    n = ctypes.c_int64(0)
    rc = fn(int(K), int(d1), indptr.ctypes.data, A.indices.ctypes.data, nz.ctypes.data, box[0].ctypes.data, box[1].ctypes.data, box[2].ctypes.data, box[3].ctypes.data, ctypes.byref(n))
    if rc != 0:
        raise ValueError(L.lib.cnmfe_last_error().decode())
    n = n.value
    return nz[:n], box[0, :n], box[1, :n], box[2, :n], box[3, :n]


def _select_rows_numpy(A, lut, nloc, cand, keep_all):
    """the same selection with index arithmetic (a scipy column slice costs more than the data it moves here)"""
    K = A.shape[1]
    nS = int(cand.size)
    if nS != K:
        starts = A.indptr[cand].astype(np.int64); lens = (A.indptr[cand + 1] - A.indptr[cand]).astype(np.int64)
        tot = int(lens.sum())
        ends = np.cumsum(lens)
        src = np.arange(tot, dtype=np.int64) + np.repeat(starts - (ends - lens), lens)
        S_indices = A.indices[src]; S_data = A.data[src]
    else:
        lens = np.diff(A.indptr).astype(np.int64)
        S_indices = A.indices; S_data = A.data
    loc = lut[S_indices]
    keep = loc >= 0
    cid = np.repeat(np.arange(nS, dtype=np.int64), lens)
    if not keep_all:
        csum = np.bincount(cid[keep], weights=S_data[keep], minlength=nS)
        sub = np.nonzero(csum > 0)[0]
        if sub.size != nS:
            colsel = np.zeros(nS, dtype=bool); colsel[sub] = True
            keep &= colsel[cid]
        ind = cand[sub]
    else:
        sub = np.arange(nS); ind = cand
    cnt = np.bincount(cid[keep], minlength=nS)[sub]
    indptr = np.zeros(sub.size + 1, dtype=np.int64); np.cumsum(cnt, out=indptr[1:])
    M = sp.csc_matrix((S_data[keep], loc[keep].astype(np.int32), indptr), shape=(nloc, sub.size))
    return ind, M

# --------------------------------------------------------------------------------------
# the blocked, GPU-resident video ( == mat_data + get_patch_data of the reference )
# --------------------------------------------------------------------------------------
class PatchedVideo:
    """Geometry of distribute_data + one resident block per owned patch.

    rank/world_size shard the patches round-robin in MATLAB's linear patch order
    (SURVEY.md section 8(e)); each rank uploads only the blocks of the patches it owns.
    """

    def __init__(self, d1, d2, T, patch_dims, ring_radius, engine: Engine, rank=0, world_size=1):
        self.d1, self.d2, self.T = int(d1), int(d2), int(T)
        self.dims = (self.d1, self.d2, self.T)
        self.w_overlap = int(ring_radius)                                  # Sources2D.m:236
        (self.nr_patch, self.nc_patch), self.patch_pos, self.block_pos = distribute_geometry(d1, d2, patch_dims, ring_radius)
        # MATLAB linear index over the nr_patch x nc_patch cell: row index fastest
        self.order = [(m, n) for n in range(self.nc_patch) for m in range(self.nr_patch)]
        self.engine = engine
        self.rank, self.world_size = rank, world_size
        self.owned = [idx for i, idx in enumerate(self.order) if i % world_size == rank]
        self.pid = {idx: i for i, idx in enumerate(self.order)}
        self.patch_pix = {idx: _rect_pixels(self.patch_pos[idx], d1) for idx in self.order}
        self.block_pix = {idx: _rect_pixels(self.block_pos[idx], d1) for idx in self.order}
        self.ind_patch = {}
        self._halo = {}
        self._lut = {}
        for idx in self.order:
            p, b = self.patch_pos[idx], self.block_pos[idx]
            mask = np.zeros((b[1] - b[0] + 1, b[3] - b[2] + 1), dtype=bool)
            mask[p[0] - b[0]:p[1] - b[0] + 1, p[2] - b[2]:p[3] - b[2] + 1] = True   # update_spatial_parallel.m:140-141
            self.ind_patch[idx] = np.nonzero(mask.reshape(-1, order="F"))[0]
        for idx in self.owned:
            engine.create_patch(self.pid[idx], self.patch_pos[idx], self.block_pos[idx], d1, d2, T)

    def lut(self, idx, kind):
        """(table, rows, (lowest, highest pixel)): global pixel -> row index inside the block / patch / halo of patch idx (-1 elsewhere), cached: lets `rows_of` slice a CSC matrix in
        O(nnz) without a CSR conversion or an index array of block length (what grows with the FOV on every rank of a sharded run)"""
        key = (idx, kind)
        t = self._lut.get(key)
        if t is None:
            pix = self.block_pix[idx] if kind == "block" else self.patch_pix[idx] if kind == "patch" else self.halo_pix(idx)
            t = np.full(self.d1 * self.d2, -1, dtype=np.int32)
            t[pix] = np.arange(pix.size, dtype=np.int32)
            t = self._lut[key] = (t, pix.size, (int(pix.min()), int(pix.max())) if pix.size else (0, -1))
        return t

    def halo_pix(self, idx):
        """block pixels outside the patch (mask==1 in update_spatial_parallel.m:84-85), cached"""
        h = self._halo.get(idx)
        if h is None:
            h = self._halo[idx] = np.setdiff1d(self.block_pix[idx], self.patch_pix[idx], assume_unique=True)
        return h

    def upload_from_full(self, Y_td, chunk=512):
        """Y_td: (T, d1*d2) host video, frame-major / pixels column-major (MATLAB d x T)."""
        for idx in self.owned:
            bp = self.block_pix[idx]
            for t0 in range(0, self.T, chunk):
                self.engine.upload_block(self.pid[idx], Y_td[t0:t0 + chunk][:, bp], t0)

    def upload_block_device(self, idx, dev_ptr):
        self.engine.upload_block_device(self.pid[idx], dev_ptr, self.T)

    # -- data plane: what distribute_data.m:56-173 + get_patch_data.m:50-93 do for the reference (blocks with their halo out of the recording).
    # The recording is read ONCE, in frame chunks; every owned block of a chunk goes up in the file's own element type (uint8/uint16/float16/
    # float32/float64: cnmfe_upload_block converts on the device) -- there is no blocked intermediate file.
    def upload_from_images(self, frames, chunk=256):
        """frames: an array (T, d1, d2) or any iterable of T images of shape (d1, d2) -- rows x columns as MATLAB's Y(:,:,t), e.g. TIFF pages.
        Pixels are re-ordered to the column-major order of the reference (pixel = (c-1)*d1 + r) chunk by chunk."""
        t0, buf = 0, []
        def flush():
            nonlocal t0, buf
            if len(buf) == 0:
                return
            arr = np.stack(buf) if not isinstance(buf, np.ndarray) else buf
            if arr.shape[1:] != (self.d1, self.d2):
                raise ValueError("frames are %s, the field of view is (%d, %d)" % (arr.shape[1:], self.d1, self.d2))
            cm = arr.transpose(0, 2, 1).reshape(arr.shape[0], self.d1 * self.d2)        # column-major pixel order
            for idx in self.owned:
                self.engine.upload_block(self.pid[idx], cm[:, self.block_pix[idx]], t0)
            t0 += arr.shape[0]; buf = []
        if isinstance(frames, np.ndarray) and frames.ndim == 3:
            for s0 in range(0, frames.shape[0], chunk):
                buf = frames[s0:s0 + chunk]; flush()
        else:
            for im in frames:
                buf.append(np.asarray(im))
                if len(buf) == chunk:
                    flush()
            flush()
        if t0 != self.T:
            raise ValueError("the recording has %d frames, the patches were created for %d" % (t0, self.T))

    def upload_from_tiff(self, path, chunk=256):
        """a multi-page TIFF (what the reference's demos ship and tif2mat.m / bigread2.m read), one page per frame"""
        from PIL import Image, ImageSequence
        with Image.open(path) as im:
            self.upload_from_images((np.asarray(page) for page in ImageSequence.Iterator(im)), chunk)

    def upload_from_raw(self, path, dtype, offset=0, order="F", chunk=256):
        """a flat binary recording of T frames (np.memmap, nothing is read twice): order='F' = MATLAB's fwrite of a d1 x d2 x T array (pixels
        column-major inside a frame), order='C' = row-major frames (rows x columns, e.g. numpy's tofile of a (T, d1, d2) array)."""
        mm = np.memmap(path, dtype=np.dtype(dtype), mode="r", offset=offset, shape=(self.T, self.d1 * self.d2))
        if order == "F":
            self.upload_from_full(mm, chunk)
        else:
            self.upload_from_images(mm.reshape(self.T, self.d1, self.d2), chunk)

    def upload_from_hdf5(self, path, dataset=None, chunk=256, frame0=0):
        """a `.h5` / `.hdf5` recording with its movie in the root group (smod_bigread2.m:338-355) or a v7.3 `.mat` recording holding `Y` or a single
        array (smod_bigread2.m:378-400).  A d1 x d2 x T MATLAB array / h5read view is the HDF5 dataset of dims (T, d2, d1) -- singleton dims anywhere, as
        in the 5-D files get_data_dimension.m:32-35 indexes with [2 3 5] -- so a hyperslab over the first axis is a run of frames already in the reference's
        pixel order.  Read once, in frame chunks; frame0 = frames to skip (obj.frame_range(1) - 1)."""
        from . import h5io
        with h5io.H5File(path) as f:
            name = dataset if dataset is not None else _pick_movie(f)
            dims = f.shape(name)
            axes = [i for i, n in enumerate(dims) if n != 1]
            if len(axes) != 3 or (dims[axes[1]], dims[axes[2]]) != (self.d2, self.d1):
                raise ValueError("dataset %r of %s has MATLAB size %s, the field of view is %d x %d" % (name, path, tuple(reversed(dims)), self.d1, self.d2))
            if frame0 < 0 or frame0 + self.T > dims[axes[0]]:
                raise ValueError("dataset %r has %d frames, frames %d..%d were asked for" % (name, dims[axes[0]], frame0 + 1, frame0 + self.T))
            f.dtype(name)                                                  # (raises for a non-numeric dataset before anything is uploaded)
            for t0 in range(0, self.T, chunk):
                n = min(chunk, self.T - t0)
                start = [0] * len(dims); count = list(dims)
                start[axes[0]], count[axes[0]] = frame0 + t0, n
                cm = f.read(name, start, count).reshape(n, self.d1 * self.d2)
                for idx in self.owned:
                    self.engine.upload_block(self.pid[idx], cm[:, self.block_pix[idx]], t0)

    def upload_from_mat_data(self, path, chunk=256, frame0=0):
        """the blocked file distribute_data.m:127-173 wrote (`mat_data`): every owned block (patch + halo) is put together from the storage blocks
        `Y_r0_r1_c0_c1` that meet it, as get_patch_data.m:50-93 does -- neighbouring storage blocks share their cut line, the shared line is the same data
        in both -- and goes up in the file's element type.  Only the parts of the file this rank's blocks cover are read."""
        from . import h5io
        with h5io.H5File(path) as f:
            info = mat_data_info(f)
            if tuple(info["dims"][:2]) != (self.d1, self.d2):
                raise ValueError("%s holds a %d x %d field of view, the patches were created for %d x %d" % ((path,) + tuple(info["dims"][:2]) + (self.d1, self.d2)))
            if frame0 < 0 or frame0 + self.T > info["dims"][2]:
                raise ValueError("%s holds %d frames, frames %d..%d were asked for" % (path, info["dims"][2], frame0 + 1, frame0 + self.T))
            stored = info["blocks"]
            for idx in self.owned:
                r0, r1, c0, c1 = [int(v) for v in self.block_pos[idx]]
                nr, nc = r1 - r0 + 1, c1 - c0 + 1
                parts = []
                for (s0, s1, q0, q1), name in stored.items():
                    a0, a1, b0, b1 = max(r0, s0), min(r1, s1), max(c0, q0), min(c1, q1)
                    if a0 <= a1 and b0 <= b1:
                        parts.append((name, (b0 - q0, a0 - s0), (b1 - b0 + 1, a1 - a0 + 1), (b0 - c0, a0 - r0)))
                cover = np.zeros((nc, nr), dtype=bool)
                for _, _, (wc, wr), (oc, orr) in parts:
                    cover[oc:oc + wc, orr:orr + wr] = True
                if not cover.all():
                    raise ValueError("%s: the stored blocks do not cover block [%d %d %d %d]" % (path, r0, r1, c0, c1))
                for t0 in range(0, self.T, chunk):
                    n = min(chunk, self.T - t0)
                    buf = np.empty((n, nc, nr), dtype=info["dtype"])
                    for name, (sc, sr), (wc, wr), (oc, orr) in parts:
                        buf[:, oc:oc + wc, orr:orr + wr] = f.read(name, (frame0 + t0, sc, sr), (n, wc, wr))
                    self.engine.upload_block(self.pid[idx], buf.reshape(n, nc * nr), t0)


def _pick_movie(f):
    """the movie of a recording: `Y` when there is one (a .mat with Y and Ysiz), else the only numeric dataset with three non-singleton dims"""
    if f.has("Y"):
        return "Y"
    cand = []
    for n in f.names():
        if f.has(n):
            try:
                f.dtype(n)
            except TypeError:
                continue
            if sum(1 for v in f.shape(n) if v != 1) == 3:
                cand.append(n)
    if len(cand) != 1:
        raise ValueError("%s: cannot tell which dataset is the movie (%s); name it" % (f.path, ", ".join(cand) or "none has three dimensions"))
    return cand[0]


def mat_data_info(f):
    """what a blocked `mat_data` file says about itself (distribute_data.m:129-158): dims, patch_dims, w_overlap, the cut lines, the element type and
    the name of every stored block keyed by its rectangle.  `f`: a path or an open h5io.H5File."""
    from . import h5io
    import re
    if not isinstance(f, h5io.H5File):
        with h5io.H5File(f) as g:
            return mat_data_info(g)
    ints = lambda name: [int(v) for v in np.asarray(f.matlab_value(name)).reshape(-1, order="F")]
    blocks = {}
    for n in f.names():
        m = re.fullmatch(r"Y_(\d+)_(\d+)_(\d+)_(\d+)", n)
        if m:
            rect = tuple(int(v) for v in m.groups())
            if f.matlab_size(n)[:2] != (rect[1] - rect[0] + 1, rect[3] - rect[2] + 1):
                raise ValueError("%s: block %s has size %s" % (f.path, n, f.matlab_size(n)))
            blocks[rect] = n
    if not blocks:
        raise ValueError("%s holds no Y_r0_r1_c0_c1 block: not a file distribute_data wrote" % f.path)
    dts = {f.dtype(n) for n in blocks.values()}
    if len(dts) != 1:
        raise ValueError("%s: the stored blocks have different element types" % f.path)
    return {"dims": tuple(ints("dims")), "patch_dims": tuple(ints("patch_dims")), "w_overlap": ints("w_overlap")[0],
            "block_idx_r": np.array(ints("block_idx_r")), "block_idx_c": np.array(ints("block_idx_c")), "dtype": dts.pop(), "blocks": blocks}


# --------------------------------------------------------------------------------------
# Sources2D
# --------------------------------------------------------------------------------------
class _LazyRow:
    """a length-K vector that arrives with a LazyHostTraces of shape (1, K) (kernel_pars, neuron_sn of deconvTemporal on the bound matrix)"""
    def __init__(self, lazy):
        self._lazy = lazy
    def __array__(self, dtype=None, copy=None):
        a = np.asarray(self._lazy)[0]
        return a.copy() if (copy or dtype is None) else a.astype(dtype)
    def __getitem__(self, k):
        return np.asarray(self._lazy)[0][k]
    def __len__(self):
        return self._lazy.shape[1]
    def __getattr__(self, name):
        if name.startswith("_"):
            raise AttributeError(name)
        return getattr(np.asarray(self._lazy)[0], name)

for _op in ("add", "sub", "mul", "truediv", "radd", "rsub", "rmul", "rtruediv", "lt", "le", "gt", "ge", "eq", "ne", "and", "rand"):
    setattr(_LazyRow, "__%s__" % _op, (lambda op: lambda self, *a: getattr(np.asarray(self._lazy)[0], "__%s__" % op)(*a))(_op))
_LazyRow.__hash__ = object.__hash__

_UNSET = object()


class _PeelSession:
    """the device's peel session of one patch as hostops.greedy_roi_block sees it"""
    def __init__(self, engine, pid, gSiz):
        self.engine, self.pid, self.gSiz = engine, pid, gSiz

    def extract(self, r, c):
        return self.engine.peel_extract(self.pid, r, c, self.gSiz)

    def apply(self, r, c, ai, Hai, ci, sig, min_pnr, min_corr):
        pnr, cn = self.engine.peel_apply(self.pid, r, c, self.gSiz, ai, Hai, ci, sig, min_pnr, min_corr)
        return pnr.astype(np.float64), cn.astype(np.float64)


class Sources2D:
    """State and the three update methods of the reference's handle class (Sources2D.m:10-57):
    A (d x K sparse), A_prev, C, C_prev, C_raw (K x T), W{.}/b0{.} (resident on the GPU per patch,
    fetch with ``get_W`` / ``get_b0``), b0_new, options, P (sn, Ymean)."""

    def __init__(self, video: PatchedVideo, options: Options, A, C, sn, dist_group=None):
        self.bg_model = str(options.background_model).lower()             # (the reference compares with strcmpi)
        if self.bg_model not in ("ring", "svd"):
            raise ValueError("only the ring and the svd background models are built; got %r" % options.background_model)
        if not (1 <= int(options.bg_ssub) <= 8):
            raise ValueError("bg_ssub must be in 1..8")
        if self.bg_model == "svd":
            self._svd_check(video.engine, options, dist_group)
        self.video = video
        self.options = options
        options.d1, options.d2 = video.d1, video.d2
        self.engine = video.engine
        d = video.d1 * video.d2
        self.A = sp.csc_matrix(A, dtype=np.float32)
        if self.A.shape[0] != d:
            raise ValueError("A must have d1*d2 rows")
        self.C = np.ascontiguousarray(C, dtype=np.float32)
        self.C_raw = self.C.copy()
        self.A_prev = self.A          # snapshots: A and C are only ever REPLACED by the update methods, never mutated in place
        self.C_prev = self.C
        self.P = {"sn": np.asarray(sn, dtype=np.float32).reshape(-1).copy(), "Ymean": {}}
        self._b0_new_val = None; self._b0_new_src = None
        self._svd_bg_fitted = False     # background_model = 'svd': b, f, b0 come from this object's own update_background_parallel (initTemporal then keeps its refusal)
        self.dist = dist_group
        # test hook: take the collective (sharded) branches even with one rank, so that a single-GPU box can run the all-gather of A, the
        # device-side stitch of C_raw and the lazy all-reduces over RCCL exactly as an N-rank job does (scripts/nccl_smoke.py)
        self.force_collectives = False
        # what one update call leaves for the next (each: who writes it; what voids it)
        self._resid_tag = {}            # patch -> who asked for its resident residual (_residual; None = anybody); a background fit of the patch drops the entry
        self._cur_blocks = {}           # patch -> (ind, A(block, ind)), cut by update_temporal_parallel under its sweeps; serves the next fit while _cur_blocks_src is self.A
        self._cur_blocks_src = None     # the A they were cut from
        self._prev_blocks = {}          # patch -> (ind, A_prev(block, ind)): filled by update_background_parallel, completed by _prev_block_of, which empties it ...
        self._prev_csr_src = None       # ... when this, the A_prev they were cut from, is no longer self.A_prev
        self._early_u = None            # (token, A): the temporal projection queued for the one-patch spatial result A; reset by every spatial launch and its taker
        self._prefetch_wanted = False   # _spatial_finish: the next search masks are to start under the temporal update's sweep call; _start_wanted_prefetch clears it
        self._ind_future = None         # (A, future of A's search masks) of _prefetch_search_location; taken by _search_location_csc, ignored unless A is self.A
        self._pool = None               # the mask thread's executor, made on first use
        self.image_ops_on_device = True # the 'dilate' masks, the circular tail, compactSpatial and trimSpatial on the engine when it declares supports_image_ops; False: hostops (same results)
        self._gather_cap = 0            # _gather_sparse: entries per rank its padded block holds; grows with the gathered counts
        self._cmean_of = None           # the C whose row means _cmean holds; any other self.C voids them
        self._init_observer = None      # tests: set to a function the two initialisations call at every step; never reset
        self._bbox_cache = ()           # _bbox_of: (matrix, bounding boxes of its columns) of the last four matrices, by identity
        self._ds_declared = (options.ssub, options.tsub)      # the down-sampling of the initialisation is declared at construction, like bg_ssub (_ds_factors)
        self._bind_C()
        self.ssub = int(options.bg_ssub) if self.bg_model == "ring" else 1      # (the svd model ignores bg_ssub, as the reference does)
        npatch = len(video.order)
        # bg_ssub > 1: every patch gets two low-resolution companions on the device (cnmfe.h, cnmfe_patch_derive)
        self.pid_fit = {idx: npatch + 2 * video.pid[idx] for idx in video.order}
        self.pid_res = {idx: npatch + 2 * video.pid[idx] + 1 for idx in video.order}
        self._ymean_full = None
        if self.bg_model == "svd":
            # initComponents_parallel.m:265-281: b{m} = zeros(nr*nc, nb), f{m} = zeros(nb, T) (and b0{m} zero); no ring, no low-resolution companions, no fit buffers
            for idx in video.owned:
                n = video.patch_pix[idx].size
                self.engine.bg_svd_set(video.pid[idx], np.zeros((n, int(options.nb))), np.zeros((int(options.nb), video.T)), np.zeros(n))
                self.P["Ymean"][idx] = self.engine.ymean(video.pid[idx])[video.ind_patch[idx]]
            return
        for idx in video.owned:                                           # initComponents_parallel.m:213-236
            self.engine.ring_init(video.pid[idx], options.ring_radius, options.num_neighbors)
            if self.ssub > 1:                                             # :214,237-251: rr = ceil(r/bg_ssub), W on the low-resolution block
                rr = -(-int(options.ring_radius) // self.ssub)
                self.engine.patch_derive(video.pid[idx], self.pid_fit[idx], self.ssub, "nearest")
                self.engine.patch_derive(video.pid[idx], self.pid_res[idx], self.ssub, "bicubic")
                self.engine.ring_init(self.pid_fit[idx], rr, options.num_neighbors)
                self.engine.ring_init(self.pid_res[idx], rr, options.num_neighbors)
            if self._can("fit_reserve"):                          # the fit's large buffers now, not inside the first update_background_parallel
                self.engine.fit_reserve(video.pid[idx] if self.ssub == 1 else self.pid_fit[idx])
            self.P["Ymean"][idx] = self.engine.ymean(video.pid[idx])[video.ind_patch[idx]]      # :338-339, patch part
        self._ymean_full = None

    @staticmethod
    def _svd_check(engine, options, dist_group):
        """background_model = 'svd': what the constructor refuses"""
        if not getattr(engine, "supports_bg_svd", False):
            raise NotImplementedError("this engine does not build background_model = 'svd' (supports_bg_svd)")
        if not (0 <= int(options.nb) <= 8):
            raise ValueError("background_model = 'svd' takes nb in 0..8, got %r" % (options.nb,))
        if dist_group is not None:
            raise NotImplementedError("background_model = 'svd' is not built for a dist_group (one rank only)")
        get = getattr(engine, "get_option", None)
        if get is not None and int(get("lanes", 1)) > 1:
            raise NotImplementedError("background_model = 'svd' is not built for lanes > 1")

    def _svd_refuse(self, what):
        """the methods that read the ring background (W, b0 on the block) are not built for the svd model"""
        if self.bg_model == "svd":
            raise NotImplementedError("%s is not built for background_model = 'svd'" % what)

    def _can(self, what):
        """the engine's class-level flag supports_<what> (engine.Engine lists them), read where the decision is made; an engine that does not declare it does not offer it"""
        return getattr(self.engine, "supports_" + what, False)

    @property
    def _sharded(self):
        """the collective branches are taken: the patches are spread over the ranks of a group (or the test hook says so)"""
        return self.dist is not None and (self.video.world_size > 1 or self.force_collectives)

    # -- accessors ------------------------------------------------------------------
    def get_W(self, idx):
        self._svd_refuse("get_W")
        return self.engine.ring_csr(self.video.pid[idx] if self.ssub == 1 else self.pid_fit[idx])

    def _slice(self, A, idx, kind, cols=None):
        """(ind, A(pixels of idx's block / patch / halo, ind)): the reference's `mask` selections (update_*_parallel.m) without a CSR of A"""
        v = self.video
        t, n, span = v.lut(idx, kind)
        cand = self._box_candidates(A, v.patch_pos[idx] if kind == "patch" else v.block_pos[idx]) if cols is None else None
        return rows_of(A, t, n, cols=cols, span=span, cand=cand)

    def _box_candidates(self, A, rect):
        """the columns of A whose bounding box meets the rectangle (block for 'block' / 'halo', patch for 'patch'): with 4 x 4 patches the first / last stored row
        test of rows_of alone passes every neuron of the patch's COLUMN band; the boxes are found once per matrix.  None: A is not a sorted CSC matrix"""
        bb = self._bbox_of(A) if sp.isspmatrix_csc(A) and A.has_sorted_indices else None
        if bb is None:
            return None
        r0, r1, c0, c1 = [int(x) - 1 for x in rect]
        nz, rmin, rmax, cmin, cmax = bb
        return nz[(rmax >= r0) & (rmin <= r1) & (cmax >= c0) & (cmin <= c1)]

    def _slice_block_patch(self, A, idx):
        """(ind, A(block, ind), A(patch, ind)) = _slice(A, idx, "block") followed by _slice(A, idx, "patch", cols=ind), in one pass over the candidates"""
        v = self.video
        cand = self._box_candidates(A, v.block_pos[idx])
        if cand is not None:
            tb, nb, _ = v.lut(idx, "block"); tp, npx, _ = v.lut(idx, "patch")
            got = _select_block_patch_native(A, tb, nb, tp, npx, cand)
            if got is not None:
                return got
        ind, A_blk = self._slice(A, idx, "block")
        return ind, A_blk, (self._slice(A, idx, "patch", cols=ind)[1] if ind.size else None)

    def _bbox_of(self, A):
        """(non-empty columns, their first / last image row and column), cached for the last few matrices by identity"""
        for M, bb in self._bbox_cache:
            if M is A:
                return bb
        bb = _bbox_native(A, self.video.d1)
        nz = np.nonzero(np.diff(A.indptr) > 0)[0] if bb is None else None
        if bb is None and nz.size == 0:
            bb = (nz, nz, nz, nz, nz)
        elif bb is None:
            d1 = self.video.d1
            rr = A.indices % d1
            starts = A.indptr[nz]
            # rows of a column are stored ascending in pixel index = image column major: first / last entry give the column range
            cmin = A.indices[starts] // d1; cmax = A.indices[A.indptr[nz + 1] - 1] // d1
            rmin = np.minimum.reduceat(rr, starts); rmax = np.maximum.reduceat(rr, starts)
            bb = (nz, rmin, rmax, cmin, cmax)
        self._bbox_cache = (self._bbox_cache + ((A, bb),))[-4:]
        return bb

    @staticmethod
    def _rows(Cm, ind):
        """Cm(ind, :) -- the matrix itself when ind is every row (so that a bound trace matrix is recognised by identity), else a
        (matrix, rows) pair that the engine resolves on the device when the matrix is the bound one"""
        return Cm if ind.size == Cm.shape[0] else BoundRows(Cm, ind)

    def _bind_C(self):
        """one upload of obj.C per iteration instead of one per engine call (cnmfe_traces_bind)"""
        if self._can("bound_traces"):
            self.engine.bind_traces(self.C)

    # -- the engine calls that come in two forms, bg_ssub = 1 and > 1: the one place that chooses --
    def _residual(self, idx, A_prev_b, C_prev_b, tag=None, want=False):
        """the background-subtraction expression of update_spatial_parallel.m:162-178 / update_temporal_parallel.m:149-165.
        tag: who asked (see _temporal_residual_early); any other request replaces it"""
        self._resid_tag[idx] = tag
        if self.ssub == 1:
            return self.engine.residual(self.video.pid[idx], A_prev_b, C_prev_b, want=want)
        return self.engine.residual_ssub(self.video.pid[idx], self.pid_res[idx], self.ssub, A_prev_b, C_prev_b, want=want)

    def _fit(self, idx, A_block, C_block):
        o, pid = self.options, self.video.pid[idx]
        if self.ssub == 1:
            return self.engine.fit_ring_model(pid, A_block, C_block, o.thresh_outlier, o.bg_acceleration, want_b0=False)         # update_background_parallel.m:218
        return self.engine.fit_ring_model_ssub(pid, self.pid_fit[idx], self.pid_res[idx], self.ssub, A_block, C_block, o.thresh_outlier, o.bg_acceleration)   # :219-230

    def _background_resident(self, idx, b0_):
        """the background of patch idx where the three readers below take it: the residual of (A_prev, C_prev) on its block (Sources2D.m:1317-1320) -- the one the
        temporal update asks for, so right after it this costs nothing --, with bg_ssub > 1 W times its 'nearest' reduction (:1325-1334), kept on the fit patch"""
        A_prev_b, C_prev_b = self._prev_block_args(idx)
        if self.ssub == 1:
            self._residual(idx, A_prev_b, C_prev_b)
        else:
            self.engine.background_ssub(self.video.pid[idx], self.pid_fit[idx], self.ssub, A_prev_b, C_prev_b, b0_[self.video.block_pix[idx]])

    def _reconstruct(self, idx, b0_, b0_new_, t0, n):
        v, eng = self.video, self.engine
        if self.ssub == 1:
            return eng.reconstruct_background(v.pid[idx], b0_[v.block_pix[idx]], b0_new_[v.patch_pix[idx]], t0, n)
        return eng.reconstruct_background_ssub(v.pid[idx], b0_new_[v.patch_pix[idx]], t0, n)

    def _rss(self, idx, A_pp, C_p, b0_, b0_new_):
        v, eng = self.video, self.engine
        if self.ssub == 1:
            return eng.compute_rss(v.pid[idx], A_pp, C_p, b0_[v.block_pix[idx]], b0_new_[v.patch_pix[idx]])
        return eng.compute_rss_ssub(v.pid[idx], A_pp, C_p, b0_new_[v.patch_pix[idx]])

    def _df_add_background(self, idx, b0_, b0_new_, A_pp, ind):
        v, eng = self.video, self.engine
        if self.ssub == 1:
            eng.df_add_background(v.pid[idx], b0_[v.block_pix[idx]], b0_new_[v.patch_pix[idx]], A_pp, ind)
        else:
            eng.df_add_background_ssub(v.pid[idx], b0_new_[v.patch_pix[idx]], A_pp, ind)

    def init_residual(self, idx):
        """@Sources2D/initComponents_residual_parallel.m:106-121,186-217 (ring model): the video greedyROI_endoscope searches for missed
        neurons in patch `idx` -- the block's neurons subtracted, then the ring background,
            Ypatch = Y(ind_patch,:) - A*C - W*(Y - A*C) - (b0 - W*mean(Y - A*C, 2))       (:199,:206; the imresize form :209-217 for bg_ssub > 1).
        The sweep over the video is cnmfe_residual[_ssub] with the block's current neurons (it leaves that residual resident, like
        the call of a temporal update would); the footprints' own A(patch,:)*C is a sparse product on the exported copy.  Returns a
        (T, d_patch) float32 array (frame-major == the reference's d x T in MATLAB order).  greedyROI_endoscope itself is host code
        outside this engine (initialisation is out of scope)."""
        self._need_data()
        self._svd_refuse("init_residual")
        ind, A_blk = self._slice(self.A, idx, "block")                                               # :116-117
        C_blk = self._rows(self.C, ind) if ind.size else None                                        # :120
        out = self._residual(idx, A_blk if ind.size else None, C_blk, want=True)
        if ind.size:
            A_pp = self._slice(self.A, idx, "patch", cols=ind)[1].tocsr()
            Cb = np.asarray(C_blk, dtype=np.float32)
            for t0 in range(0, out.shape[0], 2048):                                                  # :199, on the patch rows
                out[t0:t0 + 2048] -= (A_pp @ Cb[:, t0:t0 + 2048]).T
        return out

    def get_b0(self, idx):
        if self.bg_model == "svd":
            return self.engine.bg_svd_get(self.video.pid[idx])[2]
        return self.engine.b0(self.video.pid[idx])

    # -- background_model = 'svd': obj.b{m} (d x nb), obj.f{m} (nb x T), obj.b0{m} (d) of a patch, float64; they live on the engine --
    def get_b(self, idx):
        self._svd_only("get_b")
        return self.engine.bg_svd_get(self.video.pid[idx])[0]

    def get_f(self, idx):
        self._svd_only("get_f")
        return self.engine.bg_svd_get(self.video.pid[idx])[1]

    def set_bg_svd(self, idx, b, f, b0):
        """obj.b{idx}, obj.f{idx}, obj.b0{idx} = a saved background (another session of the same recording).  The patch's resident residual goes with the old one.
        A b{1} that is not all zero makes the next update_background_parallel a later run (its flag_first reads mean2(b{1}))."""
        self._svd_only("set_bg_svd")
        self._svd_bg_fitted = False
        n = self.video.patch_pix[idx].size
        b = np.asarray(b, dtype=np.float64).reshape(n, -1)
        if b.shape[1] > 8:
            raise ValueError("b{%s} has %d columns; at most 8" % (idx, b.shape[1]))
        self.engine.bg_svd_set(self.video.pid[idx], b, np.asarray(f, dtype=np.float64).reshape(b.shape[1], self.video.T), np.asarray(b0, dtype=np.float64).reshape(n))
        self._b0_new_src = "b0"

    def _svd_only(self, what):
        if self.bg_model != "svd":
            raise NotImplementedError("%s belongs to background_model = 'svd'" % what)

    # -- a known background on a fresh object: W{m}, b0{m} of another recording of the same field of view (there is get_W / get_b0; these are the way in) --
    def set_W(self, idx, values):
        """obj.W{idx} = values: a d x d_b sparse matrix on the ring pattern (what get_W returns; entries off the pattern are refused) or the pattern's values in
        CSR order.  The patch's resident residual goes with the old W.  The reference's first-run test (fit_ring_model.m:25: two distinct values in row 1 of
        W{m}, also update_background_parallel.m:143) then sees a FITTED W: the next update_background_parallel of this object refits from it as a later run
        and takes the "nothing changed here" skip of :188-199 for patches without neurons."""
        pat = self.get_W(idx)                                              # (refuses the svd model)
        if sp.issparse(values):
            V = sp.csr_matrix(values)
            if V.shape != pat.shape:
                raise ValueError("W{%s} is %s, got %s" % (idx, pat.shape, V.shape))
            rows = np.repeat(np.arange(pat.shape[0]), np.diff(pat.indptr))
            vals = np.asarray(V[rows, pat.indices]).ravel().astype(np.float32)
            if np.count_nonzero(vals) != V.count_nonzero():
                raise ValueError("W{%s} has entries off the ring pattern" % (idx,))
        else:
            vals = np.ascontiguousarray(values, dtype=np.float32).ravel()
            if vals.size != pat.nnz:
                raise ValueError("W{%s} has %d entries on its ring pattern, got %d values" % (idx, pat.nnz, vals.size))
        for pid in ([self.video.pid[idx]] if self.ssub == 1 else [self.pid_fit[idx], self.pid_res[idx]]):
            self.engine.ring_set_values(pid, vals)
        self._resid_tag.pop(idx, None)

    def set_b0(self, idx, b0):
        """obj.b0{idx} = b0 (the patch's pixels, column-major).  Beside a W from set_W this completes a transplanted background: the first-run test of
        fit_ring_model.m:25 looks at W alone and then sees a fitted one.  The patch's resident residual goes with the old b0; b0_new is re-read from b0."""
        self._svd_refuse("set_b0 (use set_bg_svd)")
        b0 = np.ascontiguousarray(b0, dtype=np.float32).ravel()
        if b0.size != self.video.patch_pix[idx].size:
            raise ValueError("b0{%s} has %d pixels, got %d" % (idx, self.video.patch_pix[idx].size, b0.size))
        self.engine.set_b0(self.video.pid[idx], b0)
        self._resid_tag.pop(idx, None)
        self._b0_new_src = "b0"

    # obj.A_raw: the spatial update before post-processing.  Nothing in the iteration reads it, so the one-patch path stores the recipe (a callable) and
    # the matrix is assembled on first read
    @property
    def A_raw(self):
        v = self.__dict__.get("_A_raw")
        if callable(v):
            v = self.__dict__["_A_raw"] = v()
        return v

    @A_raw.setter
    def A_raw(self, val):
        self.__dict__["_A_raw"] = val

    # how many patches' spatial results may be outstanding before the oldest is collected: the host queues that many patches ahead of the device (each
    # result waits in a pinned buffer of its size; a lag of 1 tied the host to the device's pace and left the device idle whenever a patch's host work ran long)
    spatial_lag = 16
    _bbox_cache = ()                # (before __init__ has run, as on an object made with __new__: nothing cached yet)

    def _need_data(self):
        if self.video is None:
            raise RuntimeError("No data file selected")                   # update_spatial_parallel.m:13-38

    def estimate_noise(self, frame_range=None):
        """obj.P.sn = obj.estimate_noise(frame_range, 'psd')  (Sources2D.m:328-379): GetSn per pixel on the device (every owned patch evaluates its
        block, the patch part is kept), then the storage-block bookkeeping of :361-376.  frame_range = (1, n): the first n frames."""
        self._need_data()
        v = self.video
        n = None if frame_range is None else int(frame_range[1]) - int(frame_range[0]) + 1
        if frame_range is not None and int(frame_range[0]) != 1:
            raise NotImplementedError("estimate_noise reads the frames from the first one on (the reference's default is [1, min(T, 3000)])")
        out = np.zeros(v.d1 * v.d2, dtype=np.float64)
        for idx in v.owned:
            out[v.patch_pix[idx]] = self.engine.estimate_noise(v.pid[idx], n)[v.ind_patch[idx]]
        out = self._allreduce(out).reshape(v.d1, v.d2, order="F")
        pr = np.array([int(v.patch_pos[(m, 0)][0]) for m in range(v.nr_patch)] + [v.d1])       # patch_idx_r / patch_idx_c of distribute_data.m:57-79
        pc = np.array([int(v.patch_pos[(0, j)][2]) for j in range(v.nc_patch)] + [v.d2])
        sn = estimate_noise_image(out, storage_block_index(v.d1, pr, v.w_overlap), storage_block_index(v.d2, pc, v.w_overlap))
        self.P["sn"] = sn.reshape(-1, order="F").astype(np.float32)
        return sn

    def correlation_pnr_parallel(self, frame_range=None):
        """[Cn, PNR] = obj.correlation_pnr_parallel(frame_range)  (@Sources2D/correlation_pnr_parallel.m:1-128): the local-correlation and peak-to-noise images
        of the spatially filtered video, d1 x d2 float64 each.  Every owned patch evaluates its block on the device (Engine.seed_images) and keeps the patch
        interior (:117-127: the interiors are disjoint, so the reference's max merge is a scatter; sharded runs sum them).  frame_range = (1, n), 1-based
        inclusive and clipped to the recording as in :40-45.
        options.ssub / options.tsub other than 1 (:81-100): every block is down-sampled on the device first (Engine.seed_images_ds: dsData), filtered with the
        kernel of gSig / ssub and ceil(gSiz / ssub), detrended against the basis of the Ts = floor(n / tsub) frames that are left, and with ssub > 1 both images
        are resized back to the block (imresize, bicubic) before the patch interior is kept."""
        self._need_data()
        v, o = self.video, self.options
        nk = int(o.nk)
        if nk > 1 and str(o.detrend_method).lower() != "spline":
            raise NotImplementedError("correlation_pnr_parallel: detrend_method %r is not built (only 'spline')" % (o.detrend_method,))
        f0, f1 = (1, v.T) if frame_range is None or len(frame_range) == 0 else (int(frame_range[0]), int(frame_range[1]))
        f0, f1 = min(max(f0, 1), v.T), min(max(f1, 1), v.T)
        if f0 != 1:
            raise NotImplementedError("correlation_pnr_parallel reads the frames from the first one on (frame_range = [%d, %d])" % (f0, f1))
        n = f1 - f0 + 1
        ssub, tsub = self._ds_factors(n)
        ds = ssub != 1 or tsub != 1
        psf = seed_psf(float(o.gSig) / ssub, float(np.ceil(float(o.gSiz) / ssub)), bool(o.center_psf))      # :81-82
        Q = np.linalg.qr(bspline_basis(n // tsub, nk))[0] if nk > 1 else None     # detrend_data.m:23-29: the projection only needs the span
        Cn = np.zeros(v.d1 * v.d2, dtype=np.float64); PNR = np.zeros(v.d1 * v.d2, dtype=np.float64)
        for idx in v.owned:
            if ds:
                bp = v.block_pos[idx]
                nr_b, nc_b = int(bp[1] - bp[0] + 1), int(bp[3] - bp[2] + 1)
                cn_b, pnr_b = self.engine.seed_images_ds(v.pid[idx], ssub, tsub, psf, n, Q, 3.0)
                if ssub != 1:                                              # :97-100
                    d1s, d2s = -(-nr_b // ssub), -(-nc_b // ssub)
                    cn_b, pnr_b = (hostops.imresize_to(x.astype(np.float64).reshape(d1s, d2s, order="F"), (nr_b, nc_b)).reshape(-1, order="F") for x in (cn_b, pnr_b))
            else:
                cn_b, pnr_b = self.engine.seed_images(v.pid[idx], psf, n, Q, 3.0)
            Cn[v.patch_pix[idx]] = cn_b[v.ind_patch[idx]]
            PNR[v.patch_pix[idx]] = pnr_b[v.ind_patch[idx]]
        both = self._allreduce(np.stack([Cn, PNR]))
        return both[0].reshape(v.d1, v.d2, order="F"), both[1].reshape(v.d1, v.d2, order="F")

    def _ds_factors(self, n):
        """(ssub, tsub) of the options, checked: ssub an integer in 1..8, tsub an integer >= 1, and with either other than 1 at least 64 of the n frames left
        (ValueError with the numbers).  Factors other than 1 are honoured where the object was CONSTRUCTED with them, as bg_ssub is read at construction: an
        options object swapped in later with other factors is refused (NotImplementedError), and so is an engine that does not declare the down-sampled entry
        points (Engine.supports_init_ds) -- both before the frame count is looked at."""
        ssub, tsub = self.options.ssub, self.options.tsub
        if isinstance(ssub, bool) or ssub != int(ssub) or not (1 <= int(ssub) <= 8):
            raise ValueError("options.ssub must be an integer in 1..8, got %r" % (ssub,))
        if isinstance(tsub, bool) or tsub != int(tsub) or int(tsub) < 1:
            raise ValueError("options.tsub must be an integer >= 1, got %r" % (tsub,))
        ssub, tsub = int(ssub), int(tsub)
        if ssub != 1 or tsub != 1:
            declared = getattr(self, "_ds_declared", (1, 1))
            if (ssub, tsub) != declared:
                raise NotImplementedError("ssub = %d, tsub = %d were set after the object was constructed with ssub = %s, tsub = %s: other factors need a new Sources2D"
                                          % (ssub, tsub, declared[0], declared[1]))
            if not self._can("init_ds"):
                raise NotImplementedError("this engine does not build ssub / tsub other than 1 (supports_init_ds)")
        if (ssub != 1 or tsub != 1) and n // tsub < 64:
            raise ValueError("options.tsub = %d leaves floor(%d / %d) = %d frames, at least 64 are needed" % (tsub, n, tsub, n // tsub))
        return ssub, tsub

    def _init_deconv(self):
        """the deconvolution of one accepted trace (greedyROI_endoscope.m:355-364) both initialisations hand to hostops.greedy_roi_block: ci_raw -> (ci, ci_raw - b,
        si, kernel parameter), or None without deconv_flag"""
        o = self.options
        if not o.deconv_flag:
            return None

        def deconv(ci_raw):
            c_, r_, s_, kp_, _sn = self.engine.deconv_temporal(np.asarray(ci_raw, dtype=np.float64)[None, :], o.deconv_options)      # (the engine rounds to fp32 at the ABI)
            return c_[0].astype(np.float64), r_[0].astype(np.float64), s_[0].astype(np.float64), float(kp_[0])
        return deconv

    def _init_upsample(self, res, ssub, tsub, low, full, n):
        """greedyROI_endoscope.m:464-487: the result of hostops.greedy_roi_block on the low-resolution session brought back to the block and to n frames"""
        k = len(res["A"])
        out = dict(res)
        if ssub != 1:
            A = []
            for (r0, r1, c0, c1), ai in res["A"]:
                img = np.zeros(low)
                img[r0:r1, c0:c1] = ai
                A.append(((0, full[0], 0, full[1]), hostops.imresize_to(img, full)))       # :467 (bicubic; negative lobes kept)
            out["A"] = A
            out["center"] = res["center"] * ssub - 1                                       # :473
        if tsub != 1 and k:
            Ts = len(res["C"][0])
            Mbox = hostops.imresize_matrix(Ts, n, "box")                                    # :481-482
            out["C"] = [Mbox @ np.asarray(c, dtype=np.float64) for c in res["C"]]
            out["C_raw"] = [Mbox @ np.asarray(c, dtype=np.float64) for c in res["C_raw"]]
            if self.options.deconv_flag:
                Mcub = hostops.imresize_matrix(Ts, n, "bicubic")                            # :484
                out["S"] = [Mcub @ np.asarray(s, dtype=np.float64) for s in res["S"]]
        return out

    def _stitch_init(self, per_patch, n):
        """the collection both initialisations share (initComponents_parallel.m:410-469, initComponents_residual_parallel.m:345-398): per_patch[idx] = (the
        result of hostops.greedy_roi_block, the neurons of it that are kept, the 1-based FOV position (r0, c0) of the rectangle the result's coordinates refer to);
        patches in column-major order, neurons by discovery.  Sharded: one all-reduce of the counts, the all-gather of A, one all-reduce of the packed rows.
        Returns (A d x K csc, C, C_raw, S (K x n float32), kernel_pars, center (K x 2, 1-based FOV))."""
        v, o = self.video, self.options
        d = v.d1 * v.d2
        sharded = self._sharded
        counts = np.zeros(len(v.order), dtype=np.int64)
        for i, idx in enumerate(v.order):
            if idx in per_patch:
                counts[i] = len(per_patch[idx][1])
        if sharded:
            counts = np.rint(self._allreduce(counts.astype(np.float64))).astype(np.int64)
        first = np.concatenate([[0], np.cumsum(counts)])                  # :466-469: patches in column-major order, neurons by discovery
        Ktot = int(first[-1])
        rows, cols, vals = [], [], []
        Cm = np.zeros((Ktot, n), dtype=np.float32); Craw = np.zeros((Ktot, n), dtype=np.float32); Sm = np.zeros((Ktot, n), dtype=np.float32)
        kp = np.zeros(Ktot, dtype=np.float64); center = np.zeros((Ktot, 2), dtype=np.float64)
        for i, idx in enumerate(v.order):
            if idx not in per_patch:
                continue
            res, keep, (br0, bc0) = per_patch[idx]
            for j, k in enumerate(keep):
                col = int(first[i]) + j
                (r0, r1, c0, c1), ai = res["A"][k]
                rr, cc = np.nonzero(ai)
                rows.append((cc + c0 + bc0 - 1) * v.d1 + (rr + r0 + br0 - 1)); cols.append(np.full(rr.size, col)); vals.append(ai[rr, cc])
                Cm[col] = res["C"][k]; Craw[col] = res["C_raw"][k]
                if o.deconv_flag:
                    Sm[col] = res["S"][k]; kp[col] = res["kernel_pars"][k]
                center[col] = (res["center"][k, 0] + br0 - 1, res["center"][k, 1] + bc0 - 1)      # :461
        A = (sp.csc_matrix((np.concatenate(vals).astype(np.float32), (np.concatenate(rows), np.concatenate(cols))), shape=(d, Ktot)) if rows
             else sp.csc_matrix((d, Ktot), dtype=np.float32))
        if sharded:
            A = sp.csc_matrix(self._gather_sparse(A), dtype=np.float32)
            pack = self._allreduce(np.concatenate([Cm, Craw, Sm, kp[:, None].astype(np.float32), center.astype(np.float32)], axis=1))
            Cm, Craw, Sm = (np.ascontiguousarray(pack[:, i * n:(i + 1) * n]) for i in range(3))
            kp, center = pack[:, 3 * n].astype(np.float64), pack[:, 3 * n + 1:3 * n + 3].astype(np.float64)
        return A, Cm, Craw, Sm, kp, center

    def initComponents_parallel(self, K=None, frame_range=None, seeds=None, use_prev=False, save_avi=False, debug_on=False):
        """[center, Cn, PNR] = obj.initComponents_parallel(K, frame_range, save_avi, use_parallel, use_prev)  (@Sources2D/initComponents_parallel.m:200-203,
        308-352,410-484 -> endoscope/greedyROI_endoscope.m): the greedy initialisation of every owned patch on the device's peel session of its block
        (Engine.peel_open / peel_extract / peel_apply), the search loop and the single-image / single-trace work on the host in float64
        (hostops.greedy_roi_block).  Sets A, C, C_raw, S, P.kernel_pars (deconv_flag), Cn, ids, tags, P.Ymean and returns (center, Cn, PNR) in FOV coordinates
        (1-based).  K: the maximum number of neurons PER PATCH (None: options.K).  frame_range = (1, n).
        seeds: a list of 1-based FOV pixels (r, c), the counterpart of seed_method = 'manual': min_corr and min_pnr are halved (:66-69), and every patch tries
        the given pixels of its block ONCE, in the given order -- the one deviation: the reference asks for another round of clicks until none is valid.
        options.ssub / options.tsub other than 1 (greedyROI_endoscope.m:46-61,464-487): the session of every block runs on Yds = dsData(detrended block) on the
        device (Engine.peel_open_ds: ceil(nr_b / ssub) x ceil(nc_b / ssub) pixels, Ts = floor(n / tsub) frames) with gSig / ssub, gSiz = round(gSiz / ssub),
        min_pixel / ssub^2 and bd = round(bd / ssub); `seeds` land on the low-resolution pixel that holds them.  The results come back at full resolution as the
        reference brings them back: footprints, Cn and PNR by imresize (bicubic: negative lobes are kept), center = center * ssub - 1 (the reference's rule; for
        ssub >= 3 it may leave the block, and the patch-interior test is applied to it as it is), C and C_raw by imresize(., [k, n], 'box') along time, S
        bicubic; P.kernel_pars stay as fitted at the LOW frame rate, which is the reference's behaviour.
        Not built (NotImplementedError): detrend_method 'local_min', a frame range that does not start at 1, use_prev, save_avi / debug_on."""
        self._need_data()
        v, o = self.video, self.options
        nk = int(o.nk)
        if str(o.detrend_method).lower() != "spline":
            raise NotImplementedError("initComponents_parallel: detrend_method %r is not built (only 'spline')" % (o.detrend_method,))
        if use_prev:
            raise NotImplementedError("initComponents_parallel: use_prev is not built")
        if save_avi or debug_on:
            raise NotImplementedError("initComponents_parallel: save_avi / debug mode are not built")
        f0, f1 = (1, v.T) if frame_range is None or len(frame_range) == 0 else (int(frame_range[0]), int(frame_range[1]))
        f0, f1 = min(max(f0, 1), v.T), min(max(f1, 1), v.T)
        if f0 != 1:
            raise NotImplementedError("initComponents_parallel reads the frames from the first one on (frame_range = [%d, %d])" % (f0, f1))
        if seeds is None and str(o.seed_method).lower() == "manual":
            raise ValueError("seed_method = 'manual' needs the seed pixels: initComponents_parallel(seeds=[(r, c), ...])")
        n = f1 - f0 + 1
        ssub, tsub = self._ds_factors(n)
        ds = ssub != 1 or tsub != 1
        K = o.K if K is None else K
        bd = int(_mround(float(o.gSiz))) if o.bd is None else int(o.bd)   # initComponents_parallel.m:200-203
        gSiz = int(_mround(float(o.gSiz) / ssub))                         # greedyROI_endoscope.m:56-59
        min_pixel = float(o.min_pixel) / ssub ** 2
        psf = seed_psf(float(o.gSig) / ssub, float(gSiz) if ds else float(o.gSiz), bool(o.center_psf))
        Q = np.linalg.qr(bspline_basis(n, nk))[0] if nk > 1 else None     # (ssub / tsub: the FULL-LENGTH basis, the block is detrended before it is down-sampled)
        connected = bool(o.spatial_constraints.get("connected", True))
        deconv = self._init_deconv()
        d = v.d1 * v.d2
        Cn = np.zeros(d, dtype=np.float64); PNR = np.zeros(d, dtype=np.float64)
        per_patch = {}
        observer = self._init_observer                                     # tests: called with (patch idx, kind, data) at every extract / apply
        for idx in v.owned:
            pid = v.pid[idx]
            pp, bp = v.patch_pos[idx], v.block_pos[idx]
            nr_b, nc_b = int(bp[1] - bp[0] + 1), int(bp[3] - bp[2] + 1)
            d1s, d2s = -(-nr_b // ssub), -(-nc_b // ssub)                # the session's grid (the block itself without down-sampling)
            if ds:
                cn_b, pnr_b, _sn_b, yds = self.engine.peel_open_ds(pid, ssub, tsub, psf, n, Q, 3.0, want_video=observer is not None)
            else:
                cn_b, pnr_b, _sn_b = self.engine.peel_open(pid, psf, n, Q, 3.0)
            try:
                cn_s, pnr_s = cn_b.astype(np.float64).reshape(d1s, d2s, order="F"), pnr_b.astype(np.float64).reshape(d1s, d2s, order="F")
                if ds and observer is not None:
                    observer(idx, "open", dict(Cn=cn_b, PNR=pnr_b, Yds=yds))
                if ssub != 1:                                              # greedyROI_endoscope.m:471-472
                    cn_b, pnr_b = (hostops.imresize_to(x, (nr_b, nc_b)).reshape(-1, order="F") for x in (cn_s, pnr_s))
                Cn[v.patch_pix[idx]] = cn_b[v.ind_patch[idx]]
                PNR[v.patch_pix[idx]] = pnr_b[v.ind_patch[idx]]
                bd4 = [bd if int(pp[j]) == int(bp[j]) else 0 for j in range(4)]      # initComponents_parallel.m:318
                bd4 = [int(_mround(b / ssub)) for b in bd4]                # greedyROI_endoscope.m:59
                loc = None
                if seeds is not None:
                    loc = [((int(r) - int(bp[0])) // ssub, (int(c) - int(bp[2])) // ssub) for (r, c) in seeds
                           if int(bp[0]) <= int(r) <= int(bp[1]) and int(bp[2]) <= int(c) <= int(bp[3])]
                sess = _PeelSession(self.engine, pid, gSiz)
                res = hostops.greedy_roi_block(sess, cn_s, pnr_s, gSiz, psf, float(o.min_corr), float(o.min_pnr), min_pixel, bd4, K, connected, deconv, loc, 3.0,
                                               None if observer is None else (lambda kind, data, idx=idx: observer(idx, kind, data)))
            finally:
                self.engine.peel_close(pid)
            if ds:
                res = self._init_upsample(res, ssub, tsub, (d1s, d2s), (nr_b, nc_b), n)
            # initComponents_parallel.m:428-431: the neurons whose seed pixel lies in the patch interior
            ctr = res["center"]
            keep = [k for k in range(ctr.shape[0]) if int(pp[0]) <= ctr[k, 0] + int(bp[0]) - 1 <= int(pp[1]) and int(pp[2]) <= ctr[k, 1] + int(bp[2]) - 1 <= int(pp[3])]
            per_patch[idx] = (res, keep, (int(bp[0]), int(bp[2])))
        A, Cm, Craw, Sm, kp, center = self._stitch_init(per_patch, n)
        Ktot = A.shape[1]
        both = self._allreduce(np.stack([Cn, PNR]))
        Cn, PNR = both[0].reshape(v.d1, v.d2, order="F"), both[1].reshape(v.d1, v.d2, order="F")
        A.sort_indices()
        if n == v.T:
            self.set_components(A, Cm, Craw)                              # :470-472
        else:                                                             # (traces of the first n frames only: kept, but not bound for the updates)
            self.A, self.C, self.C_raw = A, Cm, Craw
            if self._can("bound_traces"):
                self.engine.bind_traces(None)
        if o.deconv_flag:                                                 # :473-480
            self.S = Sm; self.P["kernel_pars"] = kp
        else:
            self.S = np.zeros_like(Cm)
        self.Cn = Cn                                                      # :481
        self.ids = np.arange(1, Ktot + 1); self.tags = np.zeros(Ktot, dtype=np.uint16); self.P["k_ids"] = Ktot      # :482-485
        return center, Cn, PNR

    def initComponents_residual_parallel(self, K=None, min_corr=None, min_pnr=None, seed_method=None, seeds=None, save_avi=False):
        """[center, Cn, PNR] = obj.initComponents_residual_parallel(K, save_avi, use_parallel, min_corr, min_pnr, seed_method)
        (@Sources2D/initComponents_residual_parallel.m:47-64,106-121,165-220,345-412, ring model): the second pass that picks the neurons the first one missed.
        Per owned patch the residual of the block's current neurons is requested (cnmfe_residual[_ssub]), the device's peel session is opened on the PATCH and on
        Yres = Ysig - A(patch, ind) C(ind, :) (Engine.peel_open_residual), and the greedy search runs as in initComponents_parallel (hostops.greedy_roi_block)
        with bd = options.bd * [first row, last row, first column, last column of the patch grid] (:173), all frames and no detrending.  Every neuron found is
        kept (patches do not overlap); the new columns and rows are APPENDED to A, C, C_raw, S, P.kernel_pars (deconv_flag), ids continue from P.k_ids, tags
        grow by zeros (:393-412); obj.Cn, A_prev, C_prev, W and b0 stay.  Returns (center of the new neurons, Cn, PNR) in FOV coordinates (1-based), the images
        being the sessions' opening images placed by patch.  K: the maximum number of new neurons PER PATCH (None: the patch's pixel count, :61-64).
        min_corr, min_pnr, seed_method: when given they overwrite the options and stay overwritten (:47-55) -- first of all, as in the reference, so a call that is
        then refused (seed_method = 'manual' without seeds) has changed them all the same.  seeds: as in initComponents_parallel, tried by the
        patch that holds them.
        options.ssub / options.tsub other than 1 (:171-177,232 hand greedyROI_endoscope the patch residual and the options; greedyROI_endoscope.m:46-61,464-487):
        the session of every patch runs on dsData(Yres) (Engine.peel_open_residual_ds: ceil(nr / ssub) x ceil(nc / ssub) pixels of the PATCH, Ts = floor(T / tsub)
        frames; the device forms dsData(Ysig) - A_ds C_ds, no full-resolution Yres exists) with gSig / ssub, gSiz = round(gSiz / ssub), min_pixel / ssub^2, the
        filter built from the scaled values and bd = round(bd * [edge flags] / ssub) (:173, then greedyROI_endoscope.m:59); `seeds` land on the low-resolution
        cell ((r - r0) // ssub, (c - c0) // ssub) of the patch that holds them.  The results come back as in initComponents_parallel (_init_upsample): footprints,
        Cn and PNR by bicubic imresize to the patch (negative lobes kept), center = center * ssub - 1, C and C_raw by imresize(., [k, T], 'box') along time, S
        bicubic, P.kernel_pars as fitted at the LOW frame rate; a neuron is kept when its up-sampled footprint has any non-zero pixel (:362-363).  The factors are
        those the object was constructed with (_ds_factors); an engine without supports_init_residual_ds is refused, and so is a call with factors other than 1
        before any background was fitted (_first_run: the reference's second pass reads the fitted W, b0 of every patch, :186-217; on the ring's initial indicator
        the residual is no background-free video, and the down-sampled session is built for the fitted one only -- NotImplementedError).  An observer's "open" record then carries
        Yds, the (Ts, d1s d2s) video the session searches, instead of Yres.
        background_model = 'svd' (:107-122,195-199,224-227; an engine with supports_bg_svd_init_residual, else NotImplementedError): the session's block IS the patch,
        its neurons are those with any weight in the patch rectangle, and Yres = Y(patch) - A(patch, ind) C(ind, :) - (b f + b0) comes out of one pass over the
        resident video (Engine.peel_open_lowrank): no residual is requested and the updates that follow find the engine as they would have without the call.  There is
        no first-run refusal: before any fit b = f = b0 = 0 (the constructor set them) and Yres = Y - A C, as in the reference; ssub / tsub are honoured as above.
        Not built (NotImplementedError): save_avi."""
        self._need_data()
        svd = self.bg_model == "svd"
        if svd and not self._can("bg_svd_init_residual"):
            self._svd_refuse("initComponents_residual_parallel")
        v, o = self.video, self.options
        ssub, tsub = self._ds_factors(v.T)
        ds = ssub != 1 or tsub != 1
        if ds and not self._can("init_residual_ds"):
            raise NotImplementedError("this engine does not build ssub / tsub other than 1 in the second pass (supports_init_residual_ds)")
        if ds and not svd and self._first_run():                                    # W{1} is still the ring's indicator (update_background_parallel.m:143): nothing was fitted
            raise NotImplementedError("initComponents_residual_parallel with ssub / tsub other than 1 before the first update_background_parallel is not built: "
                                      "the down-sampled session needs the residual of a fitted background")
        if save_avi:
            raise NotImplementedError("initComponents_residual_parallel: save_avi is not built")
        if min_corr is not None:                                          # :47-55
            o.min_corr = float(min_corr)
        if min_pnr is not None:
            o.min_pnr = float(min_pnr)
        if seed_method is not None:
            o.seed_method = seed_method
        if seeds is None and str(o.seed_method).lower() == "manual":
            raise ValueError("seed_method = 'manual' needs the seed pixels: initComponents_residual_parallel(seeds=[(r, c), ...])")
        n = v.T
        bd = int(_mround(float(o.gSiz))) if o.bd is None else int(o.bd)   # :80-83
        gSiz = int(_mround(float(o.gSiz) / ssub))                         # greedyROI_endoscope.m:56-59
        min_pixel = float(o.min_pixel) / ssub ** 2
        psf = seed_psf(float(o.gSig) / ssub, float(gSiz) if ds else float(o.gSiz), bool(o.center_psf))
        connected = bool(o.spatial_constraints.get("connected", True))
        deconv = self._init_deconv()
        d = v.d1 * v.d2
        Cn = np.zeros(d, dtype=np.float64); PNR = np.zeros(d, dtype=np.float64)
        per_patch = {}
        observer = self._init_observer                                     # tests (the hook of initComponents_parallel): (patch idx, kind, data) at every open /
        want_video = observer is not None                                 # extract / apply; an observer is also handed the video every session was opened on
        for idx in v.owned:
            pid = v.pid[idx]
            pp = [int(x) for x in v.patch_pos[idx]]
            nr, nc = pp[1] - pp[0] + 1, pp[3] - pp[2] + 1
            d1s, d2s = -(-nr // ssub), -(-nc // ssub)                     # the session's grid (the patch itself without down-sampling)
            if svd:                                                       # :107-117 with block = patch: the neurons with any weight in the PATCH rectangle
                ind, A_pp = self._slice(self.A, idx, "patch")
                C_blk = self._rows(self.C, ind) if ind.size else None     # :120
                if not ind.size:
                    A_pp = None
            else:
                ind, A_blk = self._slice(self.A, idx, "block")            # :116-117
                C_blk = self._rows(self.C, ind) if ind.size else None     # :120
                self._residual(idx, A_blk if ind.size else None, C_blk)   # :199-217 without A(patch, ind) C: the resident Ysig (it goes with the session: tag None)
                A_pp = self._slice(self.A, idx, "patch", cols=ind)[1] if ind.size else None
            if svd:                                                       # :195-199,224-227: Y - A C - (b f + b0) in one pass, no Ysig (Engine.peel_open_lowrank)
                cn_p, pnr_p, _sn_p, yvid = self.engine.peel_open_lowrank(pid, ssub, tsub, A_pp, C_blk, psf, 3.0, want_video=want_video)
            elif ds:
                cn_p, pnr_p, _sn_p, yvid = self.engine.peel_open_residual_ds(pid, ssub, tsub, A_pp, C_blk, psf, 3.0, want_video=want_video)
            else:
                cn_p, pnr_p, _sn_p, yvid = self.engine.peel_open_residual(pid, A_pp, C_blk, psf, 3.0, want_video=want_video)
            try:
                if observer is not None:
                    observer(idx, "open", dict(Cn=cn_p, PNR=pnr_p, **({"Yds": yvid} if ds else {"Yres": yvid})))
                cn_s, pnr_s = cn_p.astype(np.float64).reshape(d1s, d2s, order="F"), pnr_p.astype(np.float64).reshape(d1s, d2s, order="F")
                if ssub != 1:                                              # greedyROI_endoscope.m:471-472
                    cn_p, pnr_p = (hostops.imresize_to(x, (nr, nc)).reshape(-1, order="F") for x in (cn_s, pnr_s))
                Cn[v.patch_pix[idx]] = cn_p
                PNR[v.patch_pix[idx]] = pnr_p
                bd4 = [bd * int(f) for f in (idx[0] == 0, idx[0] == v.nr_patch - 1, idx[1] == 0, idx[1] == v.nc_patch - 1)]      # :173
                bd4 = [int(_mround(b / ssub)) for b in bd4]                # greedyROI_endoscope.m:59
                loc = None
                if seeds is not None:
                    loc = [((int(r) - pp[0]) // ssub, (int(c) - pp[2]) // ssub) for (r, c) in seeds if pp[0] <= int(r) <= pp[1] and pp[2] <= int(c) <= pp[3]]
                sess = _PeelSession(self.engine, pid, gSiz)
                res = hostops.greedy_roi_block(sess, cn_s, pnr_s, gSiz, psf, float(o.min_corr), float(o.min_pnr), min_pixel, bd4, nr * nc if K is None else K,
                                               connected, deconv, loc, 3.0, None if observer is None else (lambda kind, data, idx=idx: observer(idx, kind, data)))
            finally:
                self.engine.peel_close(pid)
            if ds:
                res = self._init_upsample(res, ssub, tsub, (d1s, d2s), (nr, nc), n)
            keep = [k for k in range(res["center"].shape[0]) if np.any(res["A"][k][1])]      # :362-363
            per_patch[idx] = (res, keep, (pp[0], pp[2]))
        A_new, Cm, Craw, Sm, kp, center = self._stitch_init(per_patch, n)
        both = self._allreduce(np.stack([Cn, PNR]))
        Cn, PNR = both[0].reshape(v.d1, v.d2, order="F"), both[1].reshape(v.d1, v.d2, order="F")
        A_new.sort_indices()
        K_old, K_new = self.A.shape[1], A_new.shape[1]
        C_old = np.asarray(self.C, dtype=np.float32)
        Craw_old = C_old if self.C_raw is self.C else np.asarray(self.C_raw, dtype=np.float32)
        S_old = getattr(self, "S", None)
        S_old = np.asarray(S_old, dtype=np.float32) if S_old is not None and np.shape(S_old) == (K_old, n) else np.zeros((K_old, n), dtype=np.float32)
        if K_new:
            A_all = sp.hstack([sp.csc_matrix(self.A), A_new], format="csc", dtype=np.float32)                   # :393
            self.set_components(A_all, np.concatenate([C_old, Cm]), np.concatenate([Craw_old, Craw]))          # :394-395
        self.S = np.concatenate([S_old, Sm if o.deconv_flag else np.zeros_like(Cm)])                          # :396-403
        if o.deconv_flag:
            kp_old = self.P.get("kernel_pars")
            kp_old = np.asarray(kp_old, dtype=np.float64).reshape(-1) if kp_old is not None and len(kp_old) == K_old else np.zeros(K_old, dtype=np.float64)
            self.P["kernel_pars"] = np.concatenate([kp_old, kp])
        k_ids = int(self.P.get("k_ids", K_old))                           # :404-408
        ids_old = getattr(self, "ids", None)
        ids_old = np.asarray(ids_old) if ids_old is not None and len(ids_old) == K_old else np.arange(1, K_old + 1)
        tags_old = getattr(self, "tags", None)
        tags_old = np.asarray(tags_old, dtype=np.uint16) if tags_old is not None and len(tags_old) == K_old else np.zeros(K_old, dtype=np.uint16)
        self.ids = np.concatenate([ids_old, k_ids + np.arange(1, K_new + 1)]); self.tags = np.concatenate([tags_old, np.zeros(K_new, dtype=np.uint16)])
        self.P["k_ids"] = k_ids + K_new
        return center, Cn, PNR

    def reconstruct_b0(self):
        """Sources2D.m:1153-1190: stitch b0{m} into a d1 x d2 image (owned patches; all-reduced if sharded)."""
        v = self.video
        out = np.zeros(v.d1 * v.d2, dtype=np.float32)
        for idx in v.owned:
            out[v.patch_pix[idx]] = self.get_b0(idx)
        out = self._allreduce(out)
        return out.reshape(v.d1, v.d2, order="F")

    def ymean_full(self):
        if self._ymean_full is None:
            v = self.video
            out = np.zeros(v.d1 * v.d2, dtype=np.float64)
            for idx in v.owned:
                out[v.patch_pix[idx]] = self.P["Ymean"][idx]
            self._ymean_full = self._allreduce(out)
        return self._ymean_full

    def _allreduce(self, arr):
        if not self._sharded:
            return arr
        import torch
        import torch.distributed as td
        t = torch.from_numpy(np.ascontiguousarray(arr))
        if td.get_backend(self.dist) == "nccl":
            t = t.cuda()
        td.all_reduce(t, group=self.dist)
        return t.cpu().numpy()

    def _cmean(self):
        """mean(obj.C, 2), cached per C object (K x T can be hundreds of MB when many ranks share one FOV)"""
        if self._cmean_of is not self.C:
            self._cmean_val = self.C.mean(axis=1, dtype=np.float64)
            self._cmean_of = self.C
        return self._cmean_val

    def _update_b0_new(self):
        """obj.b0_new = Ymean - A*mean(C,2) (update_spatial_parallel.m:349).  Evaluated on first read from the
        (A, C) of this moment -- both are replaced, never mutated, so holding the references is a snapshot."""
        self.ymean_full()                                                 # (collective when sharded: keep it eager)
        self._b0_new_src = (self.A, self.C)

    @property
    def b0_new(self):
        if isinstance(self._b0_new_src, str):
            self._b0_new_val = self.reconstruct_b0(); self._b0_new_src = None
        if self._b0_new_src is not None:
            A, Cm = self._b0_new_src
            v = self.video
            cm = self._cmean() if Cm is self.C else Cm.mean(axis=1, dtype=np.float64)
            self._b0_new_val = (self.ymean_full() - np.asarray(A @ cm).ravel()).reshape(v.d1, v.d2, order="F")
            self._b0_new_src = None
        return self._b0_new_val

    @b0_new.setter
    def b0_new(self, val):
        self._b0_new_val, self._b0_new_src = val, None

    def set_components(self, A, C, C_raw=None):
        """Replace obj.A, obj.C (and obj.C_raw) between two update calls -- what the reference's merge / delete methods do to the handle object between
        the calls of demo_large_data_1p.m:203-209 (merge_neurons_dist_corr, merge_high_corr, remove_false_positives: not on this engine's path).  K may
        change; obj.A_prev / obj.C_prev stay what the last background update left (the reference's methods do not touch them either), so the next
        residual still subtracts the neurons the background was fitted against.  The new trace matrix is bound on the engine."""
        A = sp.csc_matrix(A, dtype=np.float32)
        C = np.ascontiguousarray(C, dtype=np.float32)
        if A.shape[0] != self.video.d1 * self.video.d2 or A.shape[1] != C.shape[0] or C.shape[1] != self.video.T:
            raise ValueError("A is %s, C is %s; expected (%d, K) and (K, %d)" % (A.shape, C.shape, self.video.d1 * self.video.d2, self.video.T))
        self.A, self.C = A, C
        self.C_raw = C if C_raw is None else np.ascontiguousarray(C_raw, dtype=np.float32)
        self._bind_C()
        self._update_b0_new()

    # -- batch mode (cnmf_e_amd/batch.py): what a parent object does to one of its batches between two update calls --
    def _set_A(self, A):
        """neuron_k.A = obj.A (initComponents_batch.m:53,97, update_spatial_batch.m:41): the footprints are replaced as a spatial update replaces them (_spatial_finish),
        the traces stay where they are -- nothing is bound or uploaded.  Everything cut from the old A is keyed by that matrix' identity (_cur_blocks_src, _ind_future,
        _bbox_cache) and lapses with it; the queued projection of a spatial result (_early_u) is dropped, b0_new is due again once C has A's K, and the next
        search masks may be prefetched.  A_prev, C_prev, W and b0 stay, as for set_components."""
        A = sp.csc_matrix(A, dtype=np.float32)
        if A.shape[0] != self.video.d1 * self.video.d2:
            raise ValueError("A must have d1*d2 rows")
        if not A.has_sorted_indices:
            A = A.copy(); A.sort_indices()
        self.A = A
        self._early_u = None
        if A.shape[1] == self.C.shape[0]:
            self._update_b0_new()
        self._prefetch_wanted = True

    def _grow_K(self, K_new):
        """neuron_k.C = [neuron_k.C; zeros(K - tmp_K, T)] (initComponents_batch.m:103-106, update_temporal_batch.m:24-27), after obj.A got its K_new columns: C, C_raw,
        S grow by zero rows, P.kernel_pars / P.neuron_sn by zeros.  When C is the engine's bound matrix and the engine offers it (supports_traces_grow) the rows are
        appended on the device (Engine.traces_grow: no K x T matrix moves, the resident C_raw / S follow); otherwise padded on the host and set_components."""
        K, T = self.C.shape
        K_new = int(K_new)
        if K_new < K:
            raise ValueError("_grow_K: %d rows asked for, C has %d" % (K_new, K))
        if K_new == K:
            return
        if self.A.shape[1] != K_new:
            raise ValueError("_grow_K: obj.A has %d columns, C is to grow to %d rows" % (self.A.shape[1], K_new))

        def pad(X):
            return np.concatenate([np.asarray(X, dtype=np.float32), np.zeros((K_new - K, T), dtype=np.float32)])
        raw_is_c = self.C_raw is self.C or self.C_raw is None
        S = getattr(self, "S", None)
        has_S = S is not None and tuple(np.shape(S)) == (K, T)
        if self._can("traces_grow") and self.C is getattr(self.engine, "_bound", None):
            live = self.engine.residents_are(self.C, self.C_raw, S if has_S else None)
            Cn, Rn, Sn = self.engine.traces_grow(K_new)
            C_raw = Cn if raw_is_c else (Rn if live else pad(self.C_raw))
            if has_S:
                self.S = Sn if live else pad(S)
            self.C, self.C_raw = Cn, C_raw
            self._update_b0_new()
        else:
            if has_S:
                self.S = pad(S)
            self.set_components(self.A, pad(self.C), None if raw_is_c else pad(self.C_raw))
        for name in ("kernel_pars", "neuron_sn"):
            val = self.P.get(name)
            if val is not None and len(val) == K:
                val = np.asarray(val).ravel()
                self.P[name] = np.concatenate([val, np.zeros(K_new - K, dtype=val.dtype)])

    def _trace_energy(self):
        """sum(obj.C.^2, 2) in float64 (update_spatial_batch.m:29), taken where C lies (Engine.trace_energy): no transfer while C is the engine's bound matrix (or a
        resident), which is how every update method leaves it; any other C goes up once as a host matrix, counted by merge_trace_uploads AND trace_matrix_uploads"""
        if self.C.shape[0] == 0:
            return np.zeros(0, dtype=np.float64)
        return self.engine.trace_energy(self.C)

    def delete(self, ind):
        """obj.delete(ind)  (@Sources2D/Sources2D.m:762-811): columns of A, rows of C / C_raw / S and of P.kernel_pars go; A_prev, C_prev stay"""
        K = self.A.shape[1]
        ind = np.atleast_1d(np.asarray(ind))
        if ind.dtype == np.bool_:                                                 # obj.delete(mask): MATLAB's usual calling style (obj.A(:, ind) = [])
            if ind.size != K:
                raise ValueError("delete: a logical index of %d entries for %d neurons" % (ind.size, K))
            ind = np.flatnonzero(ind)
        ind = ind.astype(np.int64)
        if ind.size == 0:
            return                                                                # :764-766
        if ind.min() < 0 or ind.max() >= K:
            raise IndexError("delete: neuron index out of range (0 .. %d)" % (K - 1))
        keep = np.setdiff1d(np.arange(K), ind)
        for name in ("ids", "tags"):                                              # :791-797 (the reference drops them with the neurons)
            val = getattr(self, name, None)
            if val is not None and len(val) == K:
                setattr(self, name, np.asarray(val)[keep])
        C_raw = np.asarray(self.C_raw)[keep] if self.C_raw is not None and np.asarray(self.C_raw).shape[0] == self.A.shape[1] else None
        if getattr(self, "S", None) is not None and np.asarray(self.S).shape[0] == self.A.shape[1]:
            self.S = np.asarray(self.S)[keep]                                     # :801-803
        if self.P.get("kernel_pars") is not None and len(self.P["kernel_pars"]) == self.A.shape[1]:
            self.P["kernel_pars"] = np.asarray(self.P["kernel_pars"])[keep]       # :807-809
        self.set_components(sp.csc_matrix(self.A)[:, keep], np.asarray(self.C)[keep], C_raw)   # :799-806

    # -- merging and tagging: the calls of demo_large_data_1p.m between the updates ------------------------------------
    # Shared by the three merges: the K x K criteria, graph_connected_comp and the n x n form of a group's alternation run here in float64 (hostops.py); whatever
    # is K x T -- corr(C'), corr(S'), the Gram of C_raw, the merged trace, its deconvolution, the compaction -- runs on the engine, on the matrices it holds.
    # On a sharded run every rank holds the same A, C, C_raw, S after the stitch and performs the same merge on its own engine: there is no collective, and the
    # device reductions run in a fixed order, so equal inputs give equal bits on every rank.
    def _merge_check(self, show_merge):
        if show_merge:
            raise NotImplementedError("show_merge = true (manual verification of every merge) is not built")
        self.engine._dopts(self.options.deconv_options)                         # (anything but AR(1) FOOPSI: NotImplementedError, like the other unbuilt options)

    def _trace_objs(self):
        """(C, C_raw, S or None) as the reference reads them: C_raw = C when there is none (merge_high_corr.m:24-26), S only with the right height (:57)"""
        K = self.A.shape[1]
        C_raw = self.C_raw if (self.C_raw is not None and self.C_raw.shape[0] == K) else self.C
        S = getattr(self, "S", None)
        if S is not None and (S.shape[0] != K or K == 0):
            S = None
        return self.C, C_raw, S

    def _traces_SRC(self):
        """_trace_objs() as the engine's resident matrices: nothing moves when they already are (after update_temporal_parallel with deconv_flag), else one
        cnmfe_traces_load"""
        Cm, C_raw, S = self._trace_objs()
        if Cm.shape[0] and not self.engine.residents_are(Cm, C_raw, S):
            self.engine.traces_load(Cm, C_raw, S, self.P.get("kernel_pars"))
        return Cm, C_raw, S

    def _corr_minus_eye(self, X):
        Cc = self.engine.trace_corr(X)
        return Cc - np.eye(Cc.shape[0])                                                                 # corr(C_') - eye(K)

    def _decay_ok(self, max_decay_diff):
        taud = hostops.decay_times(self.P["kernel_pars"])                                               # :74-79
        with np.errstate(invalid="ignore"):
            return np.abs(taud[:, None] - taud[None, :]) < float(max_decay_diff)

    def _centers_close(self, dmin, method_dist):
        yy, xx = hostops.neuron_centers(self.A, self.video.d1, self.video.d2, method_dist)
        return hostops.center_distances(yy, xx) <= float(np.atleast_1d(dmin)[0])

    def _merge_apply(self, groups):
        """merge_high_corr.m:116-236 without the figure: per group the alternation (hostops.merge_iterate on the Gram sub-blocks), the merged footprint, and ONE
        cnmfe_merge_apply for all merged traces, their deconvolution and obj.delete(ind_del).  Returns (merged_ROIs, newIDs), 0-based."""
        K = self.A.shape[1]
        if not groups:
            return [], np.zeros(0, dtype=np.int64)
        _, C_raw, _ = self._traces_SRC()
        Graw = self.engine.trace_corr(C_raw, raw=True)                              # C_raw C_raw': every group's G is a sub-block
        A = sp.csc_matrix(self.A).astype(np.float64)
        weights, cols = [], {}
        for IDs in groups:
            As = A[:, IDs]
            M = np.asarray((As.T @ As).todense())
            g, w = hostops.merge_iterate(Graw[np.ix_(IDs, IDs)], M)
            active = np.flatnonzero(np.asarray(As.sum(axis=1)).ravel() > 0)         # :173
            ai = np.asarray(As[active] @ g).ravel()                                 # :179 of the last round
            cols[int(IDs[0])] = (active, ai)
            weights.append(w)
        ind_del = np.zeros(K, dtype=bool)
        for IDs in groups:
            ind_del[IDs[1:]] = True                                                 # :191
        keep = np.flatnonzero(~ind_del)
        newIDs = np.flatnonzero(np.isin(keep, [int(g[0]) for g in groups]))         # :189,197-198
        Cn, Rn, Sn, kp, sn = self.engine.merge_apply(groups, weights, keep, self.options.deconv_options)
        # obj.A(active_pixel, IDs(1)) = ai (:183), then the deleted columns go (:236)
        A32 = sp.csc_matrix(self.A, dtype=np.float32)
        parts = []
        for k in keep:
            if int(k) in cols:
                active, ai = cols[int(k)]
                nz = ai != 0
                parts.append(sp.csc_matrix((ai[nz].astype(np.float32), (active[nz], np.zeros(int(nz.sum()), dtype=np.int64))), shape=(A32.shape[0], 1)))
            else:
                parts.append(A32[:, [int(k)]])
        A_new = sp.hstack(parts, format="csc").astype(np.float32)
        A_new.sort_indices()
        self._set_after_merge(A_new, keep, Cn, Rn, Sn, kp, sn, merged=newIDs)
        return [np.asarray(g) for g in groups], newIDs

    def _set_after_merge(self, A_new, keep, Cn, Rn, Sn, kp, sn, merged=None):
        """what obj.delete does to the handle's other fields (Sources2D.m:791-809), around the matrices the engine just compacted"""
        K = self.A.shape[1]
        for name in ("ids", "tags"):
            val = getattr(self, name, None)
            if val is not None and len(val) == K:
                setattr(self, name, np.asarray(val)[keep])
        had_S = getattr(self, "S", None) is not None and np.asarray(self.S).shape[0] == K
        self.A, self.C, self.C_raw = A_new, Cn, Rn
        if had_S:
            self.S = Sn
        old_kp = self.P.get("kernel_pars")
        if (old_kp is not None and len(old_kp) == K) or (merged is not None and len(merged)):
            self.P["kernel_pars"] = kp                                              # :188 (rows never deconvolved keep 0: "not yet estimated")
        if self.P.get("neuron_sn") is not None and len(self.P["neuron_sn"]) == K:
            self.P["neuron_sn"] = sn
        self._update_b0_new()

    def merge_high_corr(self, show_merge=False, merge_thr=None):
        """[merged_ROIs, newIDs] = merge_high_corr(obj, show_merge, merge_thr)  (@Sources2D/merge_high_corr.m): neurons whose footprints overlap, whose traces C
        and whose spike trains S correlate at least merge_thr = [A, C, S] are merged, component by component of that relation; a scalar is the threshold on
        corr(C') alone (:41-43), a fourth entry the largest admitted difference of the decay times (:72-81).  Without an S of the right height the spike trains
        are the thresholded differences of C_raw (:57-66), taken on the device.  Indices are 0-based; a group keeps its lowest member.
        Departures from the reference: a scalar or 4-vector argument is honoured (the reference's `numel(merge_thr) ~= 3` test at :38-40 replaces it by
        options.merge_thr); the `catch` branch that deletes a group whose deconvolution threw (:192-194) cannot occur -- the kernel raises nothing per trace; when S is
        absent it stays absent (the reference's obj.S(IDs(1), :) = ... would create one).  A merged trace without spikes gets C = C_raw - b (cnmfe.h).
        When nothing qualifies the method returns ([], []) with nothing touched and nothing rebound.
        Sharded runs: every rank holds the same A, C, C_raw, S after the stitch and performs the same merge on its own engine; there is no collective, and the
        device reductions run in a fixed order, so equal inputs give equal bits on every rank.
        Traffic: when C, C_raw and S are the engine's own (after update_temporal_parallel with deconv_flag) no K x T matrix is uploaded (counter
        merge_trace_uploads); A_prev, C_prev, W and b0 are left alone, as in the reference."""
        self._merge_check(show_merge)
        thr = np.atleast_1d(np.asarray(self.options.merge_thr if merge_thr is None else merge_thr, dtype=np.float64))
        if thr.size == 1:
            thr = np.array([0.0, thr[0], 0.0])                                      # :41-43
        if thr.size not in (3, 4):
            raise ValueError("merge_thr must be a scalar, [A, C, S] or [A, C, S, max_decay_diff]")
        K = self.A.shape[1]
        if K < 2:
            return [], np.zeros(0, dtype=np.int64)
        Cm, C_raw, S = self._trace_objs()                                           # (read where they are: the engine's own cost nothing, others one scratch upload each)
        A_overlap = hostops.footprint_overlap(self.A)                               # :52-54
        S_src = S if S is not None else self.engine.trace_diff_spikes(C_raw)        # :56-66
        S_corr = self._corr_minus_eye(S_src)                                        # :67
        C_corr = self._corr_minus_eye(Cm)                                           # :68
        with np.errstate(invalid="ignore"):
            flag = (A_overlap >= thr[0]) & (C_corr >= thr[1]) & (S_corr >= thr[2])  # :71
        if thr.size > 3:
            flag &= self._decay_ok(thr[3])                                          # :72-81
        return self._merge_apply(hostops.merge_groups(flag))

    def merge_neurons_dist_corr(self, show_merge=False, merge_thr=None, dmin=None, method_dist=None, max_decay_diff=None):
        """[merged_ROIs, newIDs] = merge_neurons_dist_corr(obj, show_merge, merge_thr, dmin, method_dist, max_decay_diff)  (@Sources2D/merge_neurons_dist_corr.m):
        neurons whose centres lie within dmin pixels (method_dist 'max': the brightest pixel, 'mean' / 'center': the centre of mass) and whose traces correlate
        at least merge_thr (a scalar; of a vector the entry for C) are merged.  Everything else as merge_high_corr, its departures included."""
        self._merge_check(show_merge)
        o = self.options
        thr = np.atleast_1d(np.asarray(o.merge_thr if merge_thr is None else merge_thr, dtype=np.float64))
        thr = float(thr[0] if thr.size == 1 else thr[1])
        K = self.A.shape[1]
        if K < 2:
            return [], np.zeros(0, dtype=np.int64)
        Cm, _, _ = self._trace_objs()
        close = self._centers_close(o.dmin if dmin is None else dmin, o.method_dist if method_dist is None else method_dist)   # :58-67
        with np.errstate(invalid="ignore"):
            flag = close & (self._corr_minus_eye(Cm) >= thr)                        # :70-73
        if max_decay_diff is not None:
            flag &= self._decay_ok(max_decay_diff)                                  # :74-82
        return self._merge_apply(hostops.merge_groups(flag))

    def merge_close_neighbors(self, show_merge=False, dmin=None, method_dist=None):
        """[merged_ROIs, newIDs] = merge_close_neighbors(obj, show_merge, dmin, method_dist)  (@Sources2D/merge_close_neighbors.m): neurons whose centres lie
        within dmin(1) pixels are merged whatever their traces do; a second entry of dmin bounds the difference of their decay times (:66-79).  Everything else
        as merge_high_corr, its departures included."""
        self._merge_check(show_merge)
        o = self.options
        dmin = np.atleast_1d(np.asarray(o.dmin if dmin is None else dmin, dtype=np.float64))
        if self.A.shape[1] < 2:
            return [], np.zeros(0, dtype=np.int64)
        flag = self._centers_close(dmin, o.method_dist if method_dist is None else method_dist)     # :49-62
        if dmin.size > 1:
            flag &= self._decay_ok(dmin[1])
        return self._merge_apply(hostops.merge_groups(flag))

    def tag_neurons_parallel(self, min_pnr=3):
        """tags_ = tag_neurons_parallel(obj, min_pnr)  (Sources2D.m:1683-1715): per neuron the sum of 1 (fewer than options.min_pixel positive pixels) and, with
        deconv_flag, 2 (no spike after the first frame), 4 (std(C_raw - C) / GetSn(C_raw) < 0.1) and 8 (max(C) / std(C_raw - C) < min_pnr).  The four per-trace
        quantities come from one kernel over the engine's C, C_raw and S (cnmfe_trace_tags); sets and returns obj.tags (uint16)."""
        A = sp.csc_matrix(self.A)
        K = A.shape[1]
        nz_pixels = np.asarray((A > 0).sum(axis=0)).ravel()                         # :1695
        tags = (nz_pixels < self.options.min_pixel).astype(np.uint16)               # :1696
        if self.options.deconv_flag and K:
            _, _, S = self._traces_SRC()
            if S is None:
                raise ValueError("tag_neurons_parallel with deconv_flag needs obj.S (run update_temporal_parallel or deconvTemporal first)")
            q = self.engine.trace_tags()
            with np.errstate(divide="ignore", invalid="ignore"):
                tags += (q[:, 3] < 1).astype(np.uint16) * 2                          # :1700-1701
                tags += (q[:, 1] / q[:, 2] < 0.1).astype(np.uint16) * 4              # :1703-1706
                tags += (q[:, 0] / q[:, 1] < min_pnr).astype(np.uint16) * 8          # :1709-1710
        self.tags = tags
        return tags

    def remove_false_positives(self, show_delete=False):
        """ids = remove_false_positives(obj)  (Sources2D.m:744-759): delete every neuron tag_neurons_parallel tagged; returns their (0-based) indices.  The rows go
        on the device (cnmfe_merge_apply without groups) when the engine holds the matrices, which it does after tag_neurons_parallel with deconv_flag."""
        if show_delete:
            raise NotImplementedError("show_delete = true (viewNeurons) is not built")
        tags = self.tag_neurons_parallel()
        ids = np.flatnonzero(tags)
        if ids.size == 0:
            return ids
        K = self.A.shape[1]
        C_raw = self.C_raw if (self.C_raw is not None and self.C_raw.shape[0] == K) else self.C
        S = getattr(self, "S", None)
        if not self.engine.residents_are(self.C, C_raw, S if (S is not None and S.shape[0] == K) else None):
            self.delete(ids)
            return ids
        keep = np.setdiff1d(np.arange(K), ids)
        Cn, Rn, Sn, kp, sn = self.engine.merge_apply([], [], keep)
        self._set_after_merge(sp.csc_matrix(self.A, dtype=np.float32)[:, keep], keep, Cn, Rn, Sn, kp, sn)
        return ids

    def deconvTemporal(self):
        """@Sources2D/deconvTemporal.m:29-105: deconvolve every row of C_raw again (fresh time constants); sets
        C, C_raw, S, P.kernel_pars, P.neuron_sn.  Rows are sharded over ranks and all-reduced when distributed."""
        K = self.C_raw.shape[0]
        if K == 0:
            return self.C_raw.copy()
        v = self.video
        rows = np.arange(K)[v.rank::v.world_size] if (self.dist is not None and v.world_size > 1) else np.arange(K)
        if rows.size == K and self._can("bound_deconv") and self.C_raw is getattr(self.engine, "_bound", None):
            # the stitched C_raw is the engine's bound matrix: deconvolved where it lies; C, C_raw - b, S come back lazily (pinned copies behind the kernels)
            C, Craw, S, kp, sn = self.engine.deconv_temporal_bound(self.options.deconv_options)
            self.C, self.C_raw, self.S = C, Craw, S
            self.P["kernel_pars"], self.P["neuron_sn"] = _LazyRow(kp), _LazyRow(sn)
            return C
        if rows.size == K:                                               # not sharded: no row gather / scatter of K x T arrays on the host
            # the ABI writes ck_raw - b into C_raw in place: only a PRIVATE plain array may be handed over -- with deconv_flag = false C_raw
            # is the same object as C / C_prev (and the engine's bound matrix), and a DeviceTraces' host cache must not diverge from its tensor
            private = (isinstance(self.C_raw, np.ndarray) and self.C_raw is not self.C and self.C_raw is not self.C_prev
                       and self.C_raw is not getattr(self.engine, "_bound", None))
            C, Craw, S, kp, sn = self.engine.deconv_temporal(self.C_raw, self.options.deconv_options, overwrite=private)
            self.C, self.C_raw, self.S = C, Craw, S
            self.P["kernel_pars"], self.P["neuron_sn"] = kp, sn
            self._bind_C()
            return C
        # rows k = rank mod world on this rank; ONE collective over the packed [C | C_raw | S | kernel_pars | sn] rows (3T + 2 floats per neuron)
        T = self.C_raw.shape[1]
        pack = np.zeros((K, 3 * T + 2), dtype=np.float32)
        if rows.size:
            c_, r_, s_, k_, n_ = self.engine.deconv_temporal(np.asarray(self.C_raw)[rows], self.options.deconv_options)
            pack[rows, :T], pack[rows, T:2 * T], pack[rows, 2 * T:3 * T], pack[rows, 3 * T], pack[rows, 3 * T + 1] = c_, r_, s_, k_, n_
        pack = self._allreduce(pack)
        C, Craw, S = (np.ascontiguousarray(pack[:, i * T:(i + 1) * T]) for i in range(3))
        kp, sn = pack[:, 3 * T].copy(), pack[:, 3 * T + 1].copy()
        self.C, self.C_raw, self.S = C, Craw, S
        self.P["kernel_pars"], self.P["neuron_sn"] = kp, sn
        self._bind_C()
        return C

    # -- background -------------------------------------------------------------------
    def update_background_parallel(self, use_parallel=True):
        """@Sources2D/update_background_parallel.m:121-146,176-230,311-317 (ring model, bg_ssub = 1; :238-242 for the svd model: _svd_update_background)."""
        self._need_data()
        if self.bg_model == "svd":
            return self._svd_update_background()
        v, o = self.video, self.options
        # the block slices of the current A: prepared by the temporal update under its GPU work when A has not changed since
        cached = self._cur_blocks_src is self.A
        infos, prefetched = {}, False
        flag_first = self._first_run()                                     # :143, from patch 1 for EVERY patch (a collective when sharded)
        self._prev_blocks = {}                                             # (ind, A_block) per patch: what the temporal update's residual needs
        for idx in v.owned:
            if cached and idx in self._cur_blocks:
                ind_nz, A_block = self._cur_blocks[idx]
            else:
                ind_nz, A_block = self._slice(self.A, idx, "block")       # :128-129
            C_block = self._rows(self.C, ind_nz)                           # :130
            self._prev_blocks[idx] = (ind_nz, A_block)
            # "stop updating B because A&C doesn't change in this area" (:188-199) is decided by the engine's
            # first-run test on W{m}(1,:) exactly like :143; an empty A_block on a later run keeps W, b0.
            if A_block.shape[1] == 0 and not flag_first:
                continue
            self._resid_tag.pop(idx, None)                                # W, b0 of this patch change: its resident residual goes with them
            if not prefetched:                                             # host thread under the first blocking (GIL-free) fit call
                self._prefetch_search_location(); prefetched = True
            if not np.isnan(o.thresh_outlier):                             # :131-138: sn of the block, resized for bg_ssub > 1
                sn_block = np.asarray(self.P["sn"], dtype=np.float32).ravel()[v.block_pix[idx]]
                if self.ssub == 1:
                    self.engine.set_noise(v.pid[idx], sn_block)
                else:
                    b = v.block_pos[idx]
                    nr_b, nc_b = int(b[1] - b[0] + 1), int(b[3] - b[2] + 1)
                    low = sn_block.reshape(nr_b, nc_b, order="F")[np.ix_(nearest_rows(nr_b, self.ssub), nearest_rows(nc_b, self.ssub))] * self.ssub
                    self.engine.set_noise(self.pid_fit[idx], low.reshape(-1, order="F"))
            _, infos[idx] = self._fit(idx, A_block if A_block.shape[1] else None, C_block)
        # :315, evaluated on first read (b0 only changes in this method), so the call returns with the fit still running on the GPU.
        # Sharded: that first read is a collective (all-reduce of the stitched image) -- like every method of this class it must then be
        # made by all ranks at the same point of the program; nobody reading it costs nothing (update_spatial_parallel replaces it).
        self._b0_new_src = "b0"
        self.A_prev = self.A                                               # :316 (no copy needed: A, C are replaced, not mutated)
        self._prev_csr_src = self.A
        self.C_prev = self.C                                               # :317
        return infos

    # -- background_model = 'svd' -------------------------------------------------------------------------------------
    def _svd_update_background(self):
        """update_background_parallel.m:121-130,145,188-199,238-242,316-317.  flag_first = (mean2(b{1}) == 0) reads patch 1 ONLY and decides for every patch, like the
        ring model's test on W{1}: a patch without a neuron in its block is skipped on every later run and keeps its b, f, b0.  nb = 0 leaves b{1} = 0 after a fit,
        so every run is then a first run, as in the reference.  DEVIATION, nb = 0 only: the reference's very FIRST call sees b{1} = zeros(nr*nc, 0), whose mean2 is NaN, so
        its flag_first is false there and patches without neurons keep b0 = 0 until a later call; here an empty b{1} counts as a first run from the start, and every
        patch gets its b0 = Ymean on the first call.  thresh_outlier and sn are dead for this model (fit_svd_model.m:29 tests a misspelt variable): not passed."""
        v, o, eng = self.video, self.options, self.engine
        b1 = eng.bg_svd_get(v.pid[v.order[0]])[0]
        flag_first = b1.size == 0 or float(np.mean(b1)) == 0.0                                       # :145
        stats = {}
        for idx in v.owned:
            ind_nz, A_block = self._slice(self.A, idx, "block")                                      # :128-129
            if A_block.shape[1] == 0 and not flag_first:                                             # :188-199
                continue
            stats[idx] = eng.bg_svd_fit(v.pid[idx], int(o.nb), A_block if A_block.shape[1] else None, self._rows(self.C, ind_nz) if ind_nz.size else None)   # :242
        self._svd_bg_fitted = True
        self._b0_new_src = "b0"
        self.A_prev = self.A                                                                         # :316
        self._prev_csr_src = self.A
        self._prev_blocks = {}
        self.C_prev = self.C                                                                         # :317
        return stats

    def _svd_update_spatial(self):
        """update_spatial_parallel.m:61-100,116-216 with tmp_block = patch_pos (:131): the neurons whose search mask meets the PATCH, the data of the patch without halo,
        Ysig = Y - (b f + b0) (:184-187), the same HALS / NNLS calls; the stitch (:320-341) is the ring model's.  No b0_new tail (:347-351 is ring-only)."""
        v, o, eng = self.video, self.options, self.engine
        if o.search_method not in ("ellipse", "dilate"):
            raise NotImplementedError("search_method must be 'ellipse' or 'dilate'")
        d, K = v.d1 * v.d2, self.A.shape[1]
        se_now = o.se
        if o.search_method == "dilate":
            o.se = None
        IND = self._search_location_csc(se_now)                                                      # :66
        trip = ([], [], [])
        for idx in v.owned:
            ind, IND_patch, A_patch, C_patch = self._spatial_masks(idx, IND)                         # :87-91
            if ind.size == 0:
                continue                                                                             # :121-124
            pp = v.patch_pix[idx]
            eng.residual_lowrank(v.pid[idx])                                                         # :184-187
            r = eng.update_spatial(v.pid[idx], o.spatial_algorithm, A_patch, C_patch, IND_patch, self.P["sn"][pp] if o.spatial_algorithm == "hals_thresh" else None,
                                   20 if o.spatial_algorithm == "nnls" else 3)                       # :203,205,211
            self._spatial_collect(trip, r, pp, ind)
        A_raw = (_csc_from_triplets(np.concatenate(trip[0]), np.concatenate(trip[1]), np.concatenate(trip[2]), (d, K)) if trip[0]
                 else sp.csc_matrix((d, K), dtype=np.float32))
        A_raw.eliminate_zeros(); A_raw.sort_indices()
        self.A_raw = A_raw
        self.A = self._post_process(A_raw) if o.spatial_constraints.get("connected", True) else A_raw   # :341
        if o.spatial_constraints.get("circular", False):
            self.A = self._circular_columns(self.A)
        self._early_u = None

    def _svd_update_temporal(self, use_c_hat):
        """update_temporal_parallel.m:74-87,112-186,264-286 with tmp_block = patch_pos (:78): the neurons that touch the PATCH, Ysig = Y - (b f + b0) (:170-173); the
        stitch over the patches (AA, :264-280) is the ring model's.  No b0_new tail (:291-295 is ring-only)."""
        v, o, eng = self.video, self.options, self.engine
        K, T = self.C.shape
        eng.stitch_begin(K, T)
        self._cur_blocks, self._cur_blocks_src = {}, None
        for idx in v.owned:
            ind, A_pp = self._slice(self.A, idx, "patch")                                            # :83-84
            if ind.size == 0:
                continue                                                                             # :123
            eng.residual_lowrank(v.pid[idx])                                                         # :170-173
            C_patch = self._rows(self.C, ind)                                                        # :86
            if not use_c_hat:
                eng.fast_temporal(v.pid[idx], A_pp, want_raw=False)                                  # :178
            elif o.deconv_flag:
                eng.hals_temporal_deconv(v.pid[idx], A_pp, C_patch, o.maxIter, o.deconv_options, want_all=None)   # :180
            else:
                eng.hals_temporal(v.pid[idx], A_pp, C_patch, o.maxIter, want_C=False, want_raw=False)
            eng.stitch_add(ind)                                                                      # :274-275
        lazy = (not o.deconv_flag) and self._can("lazy_traces")
        bound_deconv = o.deconv_flag and self._can("bound_deconv") and self._can("lazy_traces")
        self.C_raw = eng.stitch_finish(subtract_min=not o.deconv_flag, want="lazy" if lazy else ("bound" if bound_deconv else True))   # :279-280, :285
        self.C = self.deconvTemporal() if o.deconv_flag else self.C_raw                              # :282-283 / :286

    def _svd_reconstruct_background(self, f0, f1):
        """Sources2D.m:1346-1350: b f(:, frames) + b0 per patch, on the host in float64 from the fetched factors (the result is a host array anyway)"""
        v = self.video
        Ybg = np.zeros((v.d1 * v.d2, f1 - f0 + 1), dtype=np.float32)
        for idx in v.owned:
            b, f, b0 = self.engine.bg_svd_get(v.pid[idx])
            Ybg[v.patch_pix[idx]] = b @ f[:, f0 - 1:f1] + b0[:, None]
        return Ybg.reshape(v.d1, v.d2, -1, order="F")

    def _temporal_residual_early(self, idx):
        """update_temporal_parallel.m:149-152 asks for the residual of (A_prev, C_prev) on the block -- both known since the background update.
        The engine only RECORDS that request while the resident Ysig still serves the spatial update (pending footprint term), so
        the host-side part of it is done here, under the spatial sweeps that were just queued; the temporal update then finds it in place."""
        self._residual(idx, *self._prev_block_args(idx), tag=("temporal", self.A_prev, self.C_prev))

    def _temporal_residual_done(self, idx):
        t = self._resid_tag.get(idx)
        return t is not None and t[0] == "temporal" and t[1] is self.A_prev and t[2] is self.C_prev

    def _prev_block_of(self, idx):
        """(ind, A_prev(block rows, ind)) for the neurons of A_prev that touch the block (update_temporal_parallel.m:90-91); cached by
        update_background_parallel when A_prev is the A it fitted against"""
        if self._prev_csr_src is not self.A_prev:
            self._prev_csr_src = self.A_prev
            self._prev_blocks = {}
        hit = self._prev_blocks.get(idx)
        if hit is None:
            hit = self._prev_blocks[idx] = self._slice(self.A_prev, idx, "block")
        return hit

    def _prev_block_args(self, idx):
        """(A_prev(block, ind), C_prev(ind, :)) as the residual calls take them; (None, None) when no neuron of A_prev touches the block"""
        indp, A_prev_b = self._prev_block_of(idx)
        return (A_prev_b, self._rows(self.C_prev, indp)) if indp.size else (None, None)

    def _first_run(self):
        """flag_first = (length(unique(W{1}(1,:)))==2)  (update_background_parallel.m:143): the value test on patch 1's W decides the
        "nothing changed here, keep W" skip (:188-199) of EVERY patch.  Sharded: the rank that owns patch 1 evaluates it, one
        all-reduce of a flag hands it to the others (fit_ring_model's own first-run test, :25, stays per patch inside the engine)."""
        v = self.video
        idx1 = v.order[0]
        flag = float(self.engine.ring_first_run(v.pid[idx1] if self.ssub == 1 else self.pid_fit[idx1])) if idx1 in v.owned else 0.0
        return bool(self._allreduce(np.array([flag], dtype=np.float64))[0] > 0)

    # -- spatial ----------------------------------------------------------------------
    def update_spatial_parallel(self, use_parallel=True, update_sn=False):
        """@Sources2D/update_spatial_parallel.m:61-100,116-216,320-351.  Per owned patch: _spatial_inputs cuts what it reads (for every patch but the first under the
        sweeps of the patch before), _spatial_launch queues it, its values are collected at once or, from an engine that queues downloads, `spatial_lag` patches
        late (_spatial_drain); _spatial_finish stitches them into obj.A."""
        self._need_data()
        if self.bg_model == "svd":
            if update_sn:
                self._svd_refuse("update_spatial_parallel(update_sn=True)")
            return self._svd_update_spatial()
        v, o, eng = self.video, self.options, self.engine
        sn_new = np.zeros(v.d1 * v.d2, dtype=np.float64) if update_sn else None                  # :101-102
        if o.search_method not in ("ellipse", "dilate"):
            raise NotImplementedError("search_method must be 'ellipse' or 'dilate'")
        d, K = v.d1 * v.d2, self.A.shape[1]
        se_now = o.se                                                      # :56 copies the options, :63-65 clears obj.options.se: once per update, here
        if o.search_method == "dilate":
            o.se = None
        trip = ([], [], [])                                                # (rows, columns, values) of the patches collected so far
        whole_raw = whole_pp = None                                        # one patch over the whole FOV, every neuron: already A_ (and its post-processed form)
        in_flight = []                                                     # (result, patch pixels, neurons) of queued downloads not collected yet
        IND = ahead = None
        for i, idx in enumerate(v.owned):
            if IND is None:
                # the residual sweep (:162-166) does not depend on the search mask: start it (the call returns with
                # the kernel in flight) and build IND (:66) on the host underneath it
                prev = self._spatial_prev(idx)
                self._residual(idx, *prev)
                IND = self._search_location_csc(se_now)
                job = self._spatial_launch(idx, prev + self._spatial_masks(idx, IND), True, sn_new)
            else:
                job = self._spatial_launch(idx, ahead, False, sn_new)
            ahead = self._spatial_inputs(v.owned[i + 1], IND) if i + 1 < len(v.owned) else None     # the next patch's slices, cut while this patch's sweeps run
            if job is None:
                continue
            r, ind, late, whole_conn, token = job
            pp = v.patch_pix[idx]
            if late:
                in_flight.append((r, pp, ind))
                self._spatial_drain(trip, in_flight, self.spatial_lag)
                continue
            if whole_conn:
                # one patch = the field of view: post_process_spatial's connectivity constraint (:341) runs on the result where it lies
                # (an engine that queues downloads: A without stored zeros, rows sorted, and the raw update as a recipe -- see _spatial_finish)
                Anew, whole_pp = r(connected_fov=(v.d1, v.d2), **({"compact": True} if self._can("queued_fetch") else {}))
                if token:
                    self._early_u = (token, whole_pp)
            else:
                Anew = r() if self._can("lazy_traces") else r
            if pp.size == d and ind.size == K:
                whole_raw = Anew
            else:
                self._spatial_collect(trip, Anew, pp, ind)
        late_any = bool(in_flight)
        self._spatial_drain(trip, in_flight, 0)
        if late_any and self._can("synchronize"):
            # the late-collected results waited for their own point of the stream only (cnmfe_ticket_wait): what the kernels had to report (a ring over too many
            # footprints, an inconsistent table) must be heard BEFORE obj.A is replaced by what they computed
            eng.synchronize()
        if whole_raw is None:
            whole_raw = (_csc_from_triplets(np.concatenate(trip[0]), np.concatenate(trip[1]), np.concatenate(trip[2]), (d, K)) if trip[0]
                         else sp.csc_matrix((d, K), dtype=np.float32))
        self._spatial_finish(whole_raw, whole_pp, sn_new)

    def _spatial_prev(self, idx):
        """(A_prev(block, indp), C_prev(indp, :)) of the neurons a patch's residual subtracts, (None, None) without one"""
        # A_prev restricted to neurons that touch the HALO only (mask==1 after the patch is set to 2, :84-85,96)
        indp = self._slice(self.A_prev, idx, "halo")[0] if self.video.halo_pix(idx).size else np.zeros(0, dtype=np.int64)
        A_prev_b = self._slice(self.A_prev, idx, "block", cols=indp)[1] if indp.size else None   # :97
        C_prev_b = self._rows(self.C_prev, indp) if indp.size else None                         # :98
        return A_prev_b, C_prev_b

    def _spatial_masks(self, idx, IND):
        """(ind, IND(patch, ind), A(patch, ind), C(ind, :)) of the neurons whose search mask meets the patch"""
        ind, IND_patch = self._slice(IND, idx, "patch")                                          # :87, :89
        if ind.size == 0:
            return ind, IND_patch, None, None
        return ind, IND_patch, self._slice(self.A, idx, "patch", cols=ind)[1], self._rows(self.C, ind)   # :88,199 / :91

    def _spatial_inputs(self, idx, IND):
        """everything patch idx's update reads, in the order _spatial_launch takes it"""
        return self._spatial_prev(idx) + self._spatial_masks(idx, IND)

    def _spatial_launch(self, idx, inputs, residual_queued, sn_new):
        """queue patch idx's update: its residual (unless the caller has), GetSn (sn_new given: update_sn), the sweeps; with an engine that defers its results also the
        download and, under the sweeps, the temporal update's residual request.  None: no neuron in the patch.  Else (r, ind, late, whole_conn, token): r the SpatialResult
        (a blocking engine: the matrix); late: its download is queued, to be collected later; whole_conn: the patch is the field of view and the fetch applies the
        connectivity constraint; token: of the temporal projection queued behind that (0: none)."""
        v, o, eng = self.video, self.options, self.engine
        A_prev_b, C_prev_b, ind, IND_patch, A_patch, C_patch = inputs
        update_sn = sn_new is not None
        if ind.size == 0 and not update_sn:
            return None                                                                              # :121-124
        if not residual_queued:
            self._residual(idx, A_prev_b, C_prev_b)                                                  # :162-166
        pp = v.patch_pix[idx]
        sn_patch = self.P["sn"][pp]                                                                  # :90,154
        if update_sn:
            sn_patch = eng.get_sn(v.pid[idx])                                                        # :191-194  sn_patch = GetSn(Ypatch)
            sn_new[pp] = sn_patch
        if ind.size == 0:
            return None                                                                              # :196-199
        args = (v.pid[idx], o.spatial_algorithm, A_patch, C_patch, IND_patch, sn_patch if o.spatial_algorithm == "hals_thresh" else None,
                20 if o.spatial_algorithm == "nnls" else 3)                                          # :203,205,211
        if not self._can("lazy_traces"):
            return eng.update_spatial(*args), ind, False, False, 0
        r = eng.update_spatial(*args, defer=True)
        whole = pp.size == v.d1 * v.d2 and ind.size == self.A.shape[1]
        late = not whole and self._can("queued_fetch")
        whole_conn = whole and o.spatial_constraints.get("connected", True) and not self._sharded
        if late:
            # several patches: the download is queued right behind the sweeps and collected `spatial_lag` patches LATE -- a patch's values are assembled
            # on the host while the next patch's kernels, queued first, keep the device busy (a fetch per patch drained the stream 16 times per update)
            r.start()
        elif whole_conn and self._can("connected_start"):
            # one patch = the field of view: the connectivity kernel and the downloads are queued NOW, so that what the temporal update's residual request
            # starts on the device (the deferred half of the ring solve, the W*A_prev tables) runs behind them, under the host's assembly of A
            r.start_connected((v.d1, v.d2))
        self._temporal_residual_early(idx)                       # host work under the sweeps
        self._early_u, token = None, 0
        if (whole_conn and self._can("temporal_early") and not update_sn and not o.spatial_constraints.get("circular", False)
                and not o.deconv_flag and self.ssub == 1 and len(v.owned) == 1):
            # the hand-over: the temporal update's projection of this result, queued behind the connectivity kernel and the residual request above,
            # before the host has seen the values (engine option temporal_early); update_temporal_parallel claims it when self.A is still this result
            token = r.temporal_early()
        return r, ind, late, whole_conn, token

    def _spatial_collect(self, trip, A_p, pp, ind):
        coo = A_p.tocoo()
        trip[0].append(pp[coo.row]); trip[1].append(ind[coo.col]); trip[2].append(coo.data)         # :324-334 (patches are disjoint)

    def _spatial_drain(self, trip, in_flight, lag):
        """collect queued results, oldest first, until `lag` are left outstanding"""
        while len(in_flight) > lag:
            r, pp, ind = in_flight.pop(0)
            self._spatial_collect(trip, r(compact=True), pp, ind)

    def _spatial_finish(self, A_raw, A_pp, sn_new):
        """:336-351 with the update of all owned patches.  A_raw: the matrix, or -- one patch, not sharded, from an engine that compacts -- the recipe of it,
        assembled on first read (nothing in the iteration reads obj.A_raw).  A_pp: its post-processed form when the fetch applied the connectivity constraint."""
        v, o = self.video, self.options
        recipe = callable(A_raw)                                                                     # (then nothing to gather, no stored zero in A_pp)
        if not recipe:
            A_raw = self._gather_sparse(A_raw)
        if sn_new is not None:
            self.P["sn"] = self._allreduce(sn_new).astype(np.float32)                               # :336-337 (patches are disjoint)
        if not recipe:
            A_raw.eliminate_zeros(); A_raw.sort_indices()
            if A_pp is not None:
                A_pp.eliminate_zeros(); A_pp.sort_indices()
        self.A_raw = A_raw
        if A_pp is None:
            A_pp = self._post_process(A_raw) if o.spatial_constraints.get("connected", True) else A_raw      # :341, :24-26
        self.A = A_pp                                                                                # :341 (A_pp given: done with the fetch)
        if o.spatial_constraints.get("circular", False):                                            # post_process_spatial.m:28-30
            self.A = self._circular_columns(self.A)
        self._update_b0_new()                                                                        # :347-351
        # the NEXT spatial update's masks depend on this A only: their thread starts under the temporal update's blocking (GIL-free) sweep call (or the next fit call), not
        # here, where its Python would share the GIL with the temporal set-up the device waits for (0.4 ms of a rank's 4.3 at c4).  CNMFE_PREFETCH_EARLY=1, one patch: at once
        if recipe and os.environ.get("CNMFE_PREFETCH_EARLY", "0") == "1":
            self._prefetch_search_location()
        else:
            self._prefetch_wanted = True

    def _post_process(self, A_):
        """obj.post_process_spatial() (:341) works on whole footprints, which only exist after the gather.  Sharded, every rank holds the whole gathered A and
        runs the (deterministic) connectivity kernel over ALL of its columns: one 35-us kernel more per rank instead of a second all-gather round of the processed
        columns (rounds 2-5 split the columns k = rank mod world and gathered them again: two collectives + the host-side assembly of the whole A once more, on
        the spatial -> temporal hand-over where the device idles)"""
        v = self.video
        return self.engine.post_process_spatial(A_, v.d1, v.d2)

    def _image_ops_device(self, A):
        """the image operations on single footprints run on the engine: asked for (image_ops_on_device), offered (supports_image_ops), and A holds the fp32 values
        the kernels read (any other type goes through hostops, whose float64 sees every bit of it)"""
        return bool(self.image_ops_on_device) and self._can("image_ops") and A.dtype == np.float32

    def _circular_columns(self, A):
        v = self.video
        if self._image_ops_device(A):
            return self.engine.circular_constraints(A, v.d1, v.d2)
        return hostops.circular_constraints_columns(A, v.d1, v.d2)

    def compactSpatial(self):
        """obj.compactSpatial() (@Sources2D/Sources2D.m:968-974): circular_constraints on every footprint.  Replaces obj.A and nothing else: A_prev, the bound
        traces, W and b0 stay, and a search mask prefetched for the old A is not used (_search_location_csc takes a prefetch only for the A it was made from)."""
        self.A = self._circular_columns(sp.csc_matrix(self.A))

    def trimSpatial(self, thr=0.01, sz=5):
        """ind_small = obj.trimSpatial(thr, sz) (@Sources2D/Sources2D.m:942-965): every footprint keeps the 4-connected component, above thr * max, of its
        opening by a sz x sz square that holds the opening's maximum.  Replaces obj.A; returns the boolean ind_small (fewer than options.min_pixel positive
        pixels are left) and deletes nothing, as the reference (:963-964 are comments there).  sz is odd, 1 .. 9 (ValueError otherwise)."""
        v = self.video
        sz = int(sz)
        if sz < 1 or sz > 9 or sz % 2 == 0:
            raise ValueError("trimSpatial: sz = %d; the square's side is odd, 1 .. 9" % sz)
        A = sp.csc_matrix(self.A)
        min_pixel = int(np.ceil(self.options.min_pixel))                   # (a count below a fractional bound is a count below its ceiling)
        if self._image_ops_device(A):
            self.A, ind_small = self.engine.trim_spatial(A, v.d1, v.d2, thr, sz, min_pixel)
        else:
            self.A, ind_small = hostops.trim_spatial(A, v.d1, v.d2, thr, sz, min_pixel)
        return ind_small

    def _start_wanted_prefetch(self):
        if self._prefetch_wanted:
            self._prefetch_wanted = False
            self._prefetch_search_location()

    def _prefetch_search_location(self):
        """The search mask of the NEXT spatial update depends on A only, which the background update leaves alone: build it
        on a host thread while the (blocking, GIL-free) fit_ring_model call keeps the GPU busy."""
        if self.options.search_method != "ellipse":
            return
        import concurrent.futures as cf
        if self._pool is None:
            self._pool = cf.ThreadPoolExecutor(max_workers=1)
        A = self.A
        fut = self._ind_future
        if fut is not None and fut[0] is A:
            return                                                         # (already on its way: requested at the end of the spatial update that made this A)
        self._ind_future = (A, self._pool.submit(lambda: self._as_mask_csc(self._search_location_owned(A))))

    @staticmethod
    def _as_mask_csc(IND):
        M = sp.csc_matrix(IND, dtype=np.float32)
        M.sort_indices()
        return M

    def _search_location_csc(self, se=_UNSET):
        fut, self._ind_future = self._ind_future, None
        if fut is not None and fut[0] is self.A:
            return fut[1].result()
        return self._as_mask_csc(self._search_location_owned(se=se))

    def _search_location_owned(self, A=None, se=_UNSET):
        """IND = determine_search_location(obj.A, ...) (:66), evaluated only for the neurons that can reach a patch
        this rank owns (bounding box of the footprint grown by the largest possible ellipse); all other columns are
        empty here and belong to other ranks.  Single rank: every neuron."""
        v, o = self.video, self.options
        A = self.A if A is None else A
        K = A.shape[1]
        if o.search_method == "dilate":
            # update_spatial_parallel.m:56 copies the options BEFORE :63-65 clears obj.options.se: an update uses the element it finds and the
            # next one strel('disk', bSiz, 0) (determine_search_location.m:42-44).  The element is only READ here (prefetches and measurement
            # helpers call this too); update_spatial_parallel clears it once per update.  Every rank computes all columns (demo_batch_1p.m:19 and
            # demo_sfn_2018.m:19 turn 'dilate' on through with_dendrites): on the engine (footprint_ops.hpp), or with hostops -- the same index sets.
            se = o.se if se is _UNSET else se
            se = hostops.strel_disk(4) if isinstance(se, str) else hostops.strel_disk(o.bSiz) if se is None else se
            if self._image_ops_device(A):
                return self.engine.search_dilate(A, v.d1, v.d2, se, o.nb, o.nrgthr)
            return hostops.search_location_dilate(A, v.d1, v.d2, se, o.nb, o.nrgthr)
        if v.world_size == 1:
            return determine_search_location(A, v.d1, v.d2, o.min_size, o.max_size, o.dist)
        A = A.tocsc()
        reach = int(np.ceil(o.dist * o.max_size)) + 2
        cand = np.zeros(K, dtype=bool)
        nzcols = np.nonzero(np.diff(A.indptr) > 0)[0]
        rr, cc = A.indices % v.d1, A.indices // v.d1
        starts = A.indptr[nzcols]
        rmin = np.minimum.reduceat(rr, starts); rmax = np.maximum.reduceat(rr, starts)
        cmin = np.minimum.reduceat(cc, starts); cmax = np.maximum.reduceat(cc, starts)
        for idx in v.owned:
            r0, r1, c0, c1 = [int(x) - 1 for x in v.patch_pos[idx]]
            hit = (rmax + reach >= r0) & (rmin - reach <= r1) & (cmax + reach >= c0) & (cmin - reach <= c1)
            cand[nzcols[hit]] = True
        sel = np.nonzero(cand)[0]
        sub = determine_search_location(A[:, sel], v.d1, v.d2, o.min_size, o.max_size, o.dist).tocoo()
        IND = sp.csc_matrix((sub.data, (sub.row, sel[sub.col])), shape=(v.d1 * v.d2, K))
        IND.sort_indices()
        return IND

    def _gather_sparse(self, A_):
        """all-gather of the per-rank rows of A (disjoint pixel sets, no reduction).  ONE tensor collective per call once the sizes are known: every
        rank sends a padded int32 [3, cap + 1] block (row, column, value bits; the last column carries its count) with cap = the largest count of the previous
        gather + a quarter; a rank that outgrew cap is seen by everybody in the gathered counts, and everybody repeats the round with the capacity those counts ask
        for (the first call of a run costs two rounds: it starts from cap = 0)."""
        if not self._sharded:
            return A_
        import torch
        import torch.distributed as td
        coo = A_.tocoo()
        nccl = td.get_backend(self.dist) == "nccl"
        dev = torch.device("cuda", torch.cuda.current_device()) if nccl else torch.device("cpu")
        W = td.get_world_size(self.dist)                                  # (= video.world_size in a run; scripts/rank_load.py times one rank's share behind a group of one)
        n = int(coo.nnz)
        cap = self._gather_cap
        while True:
            # the padded block is put together by NumPy, not by torch CPU kernels: a torch fill / copy of this size opens an OpenMP region over every core of
            # the host, whose threads then spin -- inside a CPU-quota'd container that throttled the whole process for ~40 ms of every 100-ms scheduler period
            # (one rank of RCCL at c4: 26 -> 50-58 ms per iteration; OMP_NUM_THREADS=1 made it vanish: profiles/r04/forced_collectives.txt)
            buf_np = np.zeros((3, cap + 1), dtype=np.int32)
            m = min(n, cap)
            if n <= cap:
                buf_np[0, :m] = coo.row
                buf_np[1, :m] = coo.col
                buf_np[2, :m] = np.ascontiguousarray(coo.data, dtype=np.float32).view(np.int32)
            buf_np[0, cap] = n
            buf = torch.from_numpy(buf_np).to(dev)
            out = torch.empty((W, 3, cap + 1), dtype=torch.int32, device=dev)
            td.all_gather_into_tensor(out, buf, group=self.dist) if nccl else td.all_gather(list(out.unbind(0)), buf, group=self.dist)
            out = out.cpu().numpy()
            sizes = [int(out[w, 0, cap]) for w in range(W)]
            nmax = max(sizes)
            if nmax <= cap:
                break
            cap = ((nmax + nmax // 4 + 255) // 256) * 256                     # (the same number on every rank: it comes from the gathered counts)
        self._gather_cap = max(cap, ((nmax + nmax // 4 + 255) // 256) * 256) if nmax > (cap * 3) // 4 else cap      # (grown ahead of a matrix that fills up)
        r = np.concatenate([out[w, 0, :m_] for w, m_ in zip(range(W), sizes)])            # int32 row / column indices: the CSC build is index-bound
        c = np.concatenate([out[w, 1, :m_] for w, m_ in zip(range(W), sizes)])
        d_ = np.concatenate([np.ascontiguousarray(out[w, 2, :m_]).view(np.float32) for w, m_ in zip(range(W), sizes)])
        return _csc_from_triplets(r, c, d_, A_.shape)

    # -- objective ----------------------------------------------------------------------
    def compute_RSS(self):
        """[RSS_total, RSS] = compute_RSS(obj)  (@Sources2D/Sources2D.m:1358-1510), ring model, all frames.
        Per patch the engine needs the residual of (A_prev, C_prev) on the block (:1427-1429, :1475) -- the one the temporal update asks for, so
        right after update_temporal_parallel it is still resident (or pending) and this costs one read of Ysig per patch."""
        self._need_data()
        self._svd_refuse("compute_RSS")
        v = self.video
        b0_ = self.reconstruct_b0().reshape(-1, order="F")                                           # :1398 (a collective when sharded)
        b0_new_ = np.asarray(self.b0_new, dtype=np.float64).reshape(-1, order="F")                   # :1399
        RSS = {}
        for idx in v.owned:
            ind, _ = self._slice(self.A, idx, "block")                                              # :1423
            A_pp = self._slice(self.A, idx, "patch", cols=ind)[1] if ind.size else None              # A_patch(ind_patch, :)  (:1467)
            self._background_resident(idx, b0_)                                                      # :1427-1428, :1479-1486 ('nearest' both ways)
            RSS[idx] = self._rss(idx, A_pp, self._rows(self.C, ind) if ind.size else None, b0_, b0_new_)
        total = float(self._allreduce(np.array([sum(RSS.values())], dtype=np.float64))[0])           # :1507-1508
        self.P["RSS"] = total                                                                        # :1509
        return total, RSS

    def reconstruct_background(self, frame_range=None):
        """Ybg = reconstruct_background(obj, frame_range)  (@Sources2D/Sources2D.m:1247-1355), ring model: d1 x d2 x T' (fp32) of the
        owned patches (zeros elsewhere when sharded, like every per-patch output).  frame_range = (first, last), 1-based inclusive as in MATLAB."""
        self._need_data()
        v = self.video
        T = self.C.shape[1]
        f0, f1 = (1, T) if frame_range is None else (int(frame_range[0]), int(frame_range[1]))
        if self.bg_model == "svd":
            return self._svd_reconstruct_background(f0, f1)                                          # :1346-1350
        b0_ = self.reconstruct_b0().reshape(-1, order="F")                                           # :1292
        b0_new_ = np.asarray(self.b0_new, dtype=np.float64).reshape(-1, order="F")                   # :1293
        Ybg = np.zeros((v.d1 * v.d2, f1 - f0 + 1), dtype=np.float32)                                 # :1297
        for idx in v.owned:
            pp = v.patch_pix[idx]
            self._background_resident(idx, b0_)                                                      # :1317-1320, :1325-1334
            for t0 in range(f0 - 1, f1, 4096):                                                       # (the ABI hands out at most 65535 frames per call)
                n = min(4096, f1 - t0)
                Ybg[pp, t0 - (f0 - 1):t0 - (f0 - 1) + n] = self._reconstruct(idx, b0_, b0_new_, t0, n).T
        return Ybg.reshape(v.d1, v.d2, -1, order="F")

    def extract_DF_F_endoscope(self, Ybg=None, want_Yf=False):
        """[C_df, C_raw_df, Df] = extract_DF_F_endoscope(obj, Ybg)  (@Sources2D/Sources2D.m:540-570): the background projected onto every footprint,
        Yf = (A ./ sum(A.^2, 1))' * Ybg (:545); its baseline Df = median / prctile(Yf, df_prctile, 2) (:549-553), or with options.df_window <= T
        medfilt1(Yf, w, [], 2, 'truncate') / running_percentile(Yf(k, :), w, df_prctile) (:559, :563); C_df = C ./ Df, C_raw_df = C_raw ./ Df.  Sets nothing on the
        object, like the reference.  Df is (K,) float64 without a window and (K, T) with one; C_df, C_raw_df are float32.

        Ybg = None: the background is never assembled.  Per owned patch the residual of (A_prev, C_prev) is requested as reconstruct_background requests it, and the
        engine reconstructs and projects frame chunks on the device (df_add_background[_ssub]); a sharded run all-reduces the K x T projection once.
        Ybg given (d1 x d2 x T or d x T, the reference's argument): it goes up in frame chunks against the full-FOV A (df_add_frames).  Nothing is computed on the host.
        Raises RuntimeError where reconstruct_background would (no data, no background fit yet).

        Deviations: a row of Yf with a non-finite value (an empty footprint: 0 * Inf) has NaN throughout its Df row -- the reference's three estimators disagree with
        each other on NaN; Df is float64, C_df and C_raw_df are (float)((double)C / Df).  medfilt1 and prctile are MathWorks functions restated from their
        documentation (parity unpinned).  want_Yf = True appends Yf (K x T float64) to the result."""
        self._need_data()
        self._svd_refuse("extract_DF_F_endoscope")
        v, o, eng = self.video, self.options, self.engine
        K, T = self.C.shape
        p = float(o.df_prctile)
        w = 0 if o.df_window is None else int(o.df_window)
        if not (0.0 <= p <= 100.0) or w < 0:
            raise ValueError("df_prctile must lie in [0, 100] and df_window must not be negative")
        A = self.A if sp.isspmatrix_csc(self.A) else sp.csc_matrix(self.A)
        C_raw = self.C_raw if (self.C_raw is not None and self.C_raw.shape[0] == K) else self.C
        if Ybg is None:
            b0_ = self.reconstruct_b0().reshape(-1, order="F")                                       # :1292 (a collective when sharded)
            b0_new_ = np.asarray(self.b0_new, dtype=np.float64).reshape(-1, order="F")               # :1293
        else:
            Y = np.asarray(Ybg)
            Y = Y.reshape(-1, Y.shape[-1], order="F")
            if Y.shape != (v.d1 * v.d2, T):
                raise ValueError("Ybg has %s samples, expected %d x %d" % (Y.shape, v.d1 * v.d2, T))
        eng.df_begin(K, T)
        try:
            if Ybg is None:
                for idx in v.owned:
                    self._background_resident(idx, b0_)                                                  # :1317-1320
                    ind, A_pp = self._slice(A, idx, "patch")
                    self._df_add_background(idx, b0_, b0_new_, A_pp, ind)
                if self._sharded:                                                                        # every rank holds the sum over its own patches
                    eng.df_load(self._allreduce(eng.df_fetch()))
            elif K:
                step = max(4, min(4096, ((64 << 20) // (4 * Y.shape[0])) & ~3))
                allk = np.arange(K, dtype=np.int32)
                for t0 in range(0, T, step):
                    eng.df_add_frames(np.ascontiguousarray(Y[:, t0:t0 + step].T, dtype=np.float32), t0, A, allk)
            with np.errstate(divide="ignore"):
                inv = 1.0 / np.asarray(A.astype(np.float64).power(2).sum(axis=0)).ravel() if K else np.zeros(0)     # :545 (an empty footprint: Inf)
            return eng.df_finish(inv, p, w, self.C, C_raw, want_Yf=want_Yf)
        except Exception:
            eng.df_close()                                           # (a refused call must not leave the accumulator open)
            raise

    # -- closing calls: demo_large_data_1p.m:185,216 (orderROIs) and :229 (show_demixed_video) -------------------------------
    _ORDER_UNBUILT = {"circularity": "nnmf with a random start", "temporal_cluster": "linkage / optimalleaforder", "spatial_cluster": "linkage / optimalleaforder"}

    def _order_stats(self):
        """K x 7 per-trace statistics of (C, C_raw) where they lie (Engine.trace_order_stats): nothing moves when they are the engine's residents"""
        self._traces_SRC()
        return self.engine.trace_order_stats()

    def _order_criterion(self, srt):
        """(values, descend) of a named order, Sources2D.m:583-639; strcmpi where the reference uses it, strcmp elsewhere, anything unrecognised is 'snr' (:636)"""
        K = self.A.shape[1]
        low = srt.lower()
        for name, why in self._ORDER_UNBUILT.items():
            if srt == name or (name != "circularity" and low == name):
                raise NotImplementedError("orderROIs(%r) is not built (%s)" % (srt, why))
        A = sp.csc_matrix(self.A).astype(np.float64)
        with np.errstate(divide="ignore", invalid="ignore"):
            if low == "decay_time":                                                                       # :584-596
                kp = self.P.get("kernel_pars")
                if kp is None or len(kp) != K:
                    raise ValueError("orderROIs('decay_time') needs P['kernel_pars'] of the %d neurons (a deconvolving temporal update)" % K)
                return hostops.decay_times(kp), False
            if srt == "sparsity_spatial":                                                                 # :604-606
                return np.sqrt(np.asarray(A.power(2).sum(axis=0)).ravel()) / np.asarray(abs(A).sum(axis=0)).ravel(), False
            q = self._order_stats()
            if srt == "mean":                                                                             # :597-603
                val = q[:, 0] * np.asarray(A.sum(axis=0)).ravel()
                if not self.options.deconv_flag:
                    sn = self.P.get("neuron_sn")
                    if sn is None or len(sn) != K:
                        raise ValueError("orderROIs('mean') without deconv_flag divides by P['neuron_sn'], which this object does not hold")
                    val = val / np.asarray(sn, dtype=np.float64).ravel()
                return val, True
            if srt == "sparsity_temporal":                                                                # :607-609
                return q[:, 4] / q[:, 5], True
            if low == "pnr":                                                                              # :620-622
                return q[:, 3] / np.sqrt(q[:, 2]), True
            return q[:, 1] / q[:, 2], True                                                                # :636-638 ('snr' and everything else)

    def orderROIs(self, srt="srt"):
        """srt = orderROIs(obj, srt)  (@Sources2D/Sources2D.m:573-653): sort the neurons by 'snr' (var(C) / var(C_raw - C), descending; also any unrecognised string, as
        the reference's else), 'pnr' (max(C) / std(C_raw - C), descending), 'decay_time' (ascending), 'mean' (mean(C) * sum(A), descending; without deconv_flag
        divided by P.neuron_sn), 'sparsity_spatial' (ascending), 'sparsity_temporal' (descending), or by an explicit permutation (0-based).  Returns srt (0-based).
        MATLAB's sort rule is hostops.matlab_sort_order's.  'circularity', 'temporal_cluster' and 'spatial_cluster' raise NotImplementedError.

        The per-trace statistics come from one kernel over the engine's C and C_raw (cnmfe_trace_order_stats); the rows of C, C_raw, S, kernel_pars and sn are
        gathered on the device (cnmfe_merge_apply without groups, keep = srt), A's columns, ids, tags, P.kernel_pars and P.neuron_sn on the host.  A_prev and C_prev
        stay, as in the reference.  After a deconvolving update_temporal_parallel no K x T matrix is uploaded (counters merge_trace_uploads, trace_matrix_uploads)."""
        K = self.A.shape[1]
        if isinstance(srt, str):
            if K == 0:
                return np.zeros(0, dtype=np.int64)
            val, descend = self._order_criterion(srt)
            srt = hostops.matlab_sort_order(val, descend=descend)
        else:
            srt = np.asarray(srt)
            if srt.ndim != 1 or srt.size != K or not np.issubdtype(srt.dtype, np.integer) or not np.array_equal(np.sort(srt), np.arange(K)):
                raise ValueError("orderROIs: srt must be a permutation of 0 .. %d" % (K - 1))
            srt = srt.astype(np.int64)
        if K == 0:
            return srt
        self._traces_SRC()
        Cn, Rn, Sn, kp, sn = self.engine.merge_apply([], [], srt)
        self._set_after_merge(sp.csc_matrix(self.A, dtype=np.float32)[:, srt], srt, Cn, Rn, Sn, kp, sn)
        return srt

    def _demix_traces(self, use_craw):
        K = self.A.shape[1]
        return (self.C_raw if (self.C_raw is not None and self.C_raw.shape[0] == K) else self.C) if use_craw else self.C

    def _default_amp_ac(self, use_craw):
        """amp_ac = median(max(obj.A, [], 1)' .* max(CC, [], 2)) * 2  (show_demixed_video.m:37); max(CC, [], 2) from the engine's statistics: nothing is uploaded"""
        K = self.A.shape[1]
        if K == 0:
            return float("nan")
        q = self._order_stats()
        amax = np.asarray(sp.csc_matrix(self.A).max(axis=0).todense(), dtype=np.float64).ravel()
        return float(2.0 * np.median(amax * q[:, 6 if use_craw else 3]))

    def demixed_frames(self, kt=1, frame_range=None, amp_ac=None, use_craw=False, colors=None, chunk=100):
        """The six panels of show_demixed_video (@Sources2D/show_demixed_video.m:70-81,94-127) for the displayed frames frame_range(1) : kt : frame_range(2), as a
        generator over chunks of at most `chunk` displayed frames (the reference reloads every 100 kt frames).  Each chunk is a dict: frames (1-based), raw, bg,
        signal (raw - bg), denoised (A CC), residual (raw - bg - A CC) as d1 x d2 x n float32 and mixed as d1 x d2 x n x 3 uint16; entries outside the owned patches
        are zero when sharded, as in reconstruct_background.  Every panel of a frame is computed on the device from one read of the resident video and residual plus
        the pixel's row of A (cnmfe_demix_frames[_ssub]); nothing of d x T is assembled.
        Defaults as the reference: all frames; amp_ac = 2 median(max(A) .* max(CC)); colors (K x 3) = rows of prism(64).  Deviation: the colours are drawn once
        for the whole call by numpy.random.default_rng(0) -- the reference draws new ones with randi at every reload.
        Per patch the residual of (A_prev, C_prev) is requested once, as the temporal update requests it -- right after update_temporal_parallel the patch still
        holds it and nothing is asked for, so no trace matrix moves (bg_ssub > 1: cnmfe_background_ssub before every chunk -- the context keeps one patch's
        low-resolution background, and C_prev goes up with it); do not run an update between two chunks.
        background_model = 'svd' (an engine with supports_bg_svd_demix, else NotImplementedError): bg = b f + b0 of each patch's resident factors, in fp64 and rounded
        once (Engine.demix_frames_lowrank); no b0 image, no b0_new and no residual are formed or requested."""
        self._need_data()
        svd = self.bg_model == "svd"
        if svd and not self._can("bg_svd_demix"):
            self._svd_refuse("demixed_frames")
        v, eng = self.video, self.engine
        K, T = self.C.shape
        kt, chunk = int(kt), int(chunk)
        if kt < 1 or chunk < 1:
            raise ValueError("kt and chunk must be at least 1")
        f0, f1 = (1, T) if frame_range is None else (int(frame_range[0]), int(frame_range[1]))
        if not (1 <= f0 <= f1 <= T):
            raise ValueError("frame_range = (%d, %d) outside 1 .. %d" % (f0, f1, T))
        CC = self._demix_traces(use_craw)
        A = self.A if sp.isspmatrix_csc(self.A) else sp.csc_matrix(self.A)
        amp_ac = self._default_amp_ac(use_craw) if amp_ac is None else float(amp_ac)
        if colors is None:
            colors = hostops.prism64()[np.random.default_rng(0).integers(0, 64, size=K)]
        colors = np.asarray(colors, dtype=np.float32).reshape(-1, 3)
        if colors.shape[0] != K:
            raise ValueError("colors must be %d x 3" % K)
        mix_scale = 2.0 / amp_ac * 65536.0 if K else 0.0
        if not svd:
            b0_ = self.reconstruct_b0().reshape(-1, order="F")                                       # (a collective when sharded)
            b0_new_ = np.asarray(self.b0_new, dtype=np.float64).reshape(-1, order="F")
        frames = np.arange(f0, f1 + 1, kt)
        cut = {idx: self._slice(A, idx, "patch") for idx in v.owned}
        names = ("raw", "bg", "signal", "denoised", "residual")
        for c0 in range(0, frames.size, chunk):
            fr = frames[c0:c0 + chunk]
            n = fr.size
            out = {k: np.zeros((v.d1 * v.d2, n), dtype=np.float32) for k in names}
            mixed = np.zeros((v.d1 * v.d2, n, 3), dtype=np.uint16)
            for idx in v.owned:
                pp = v.patch_pix[idx]
                ind, A_pp = cut[idx]
                if svd:
                    res = eng.demix_frames_lowrank(v.pid[idx], A_pp if ind.size else None, CC, ind, colors[ind], mix_scale, int(fr[0]) - 1, kt, n)
                else:
                    if self.ssub > 1:
                        self._background_resident(idx, b0_)
                    elif not self._temporal_residual_done(idx):              # (right after update_temporal_parallel the patch still holds that residual: nothing to ask for)
                        self._temporal_residual_early(idx)
                    res = eng.demix_frames(v.pid[idx], b0_[v.block_pix[idx]] if self.ssub == 1 else None, b0_new_[pp], A_pp if ind.size else None, CC, ind,
                                           colors[ind], mix_scale, int(fr[0]) - 1, kt, n)
                for k in names:
                    out[k][pp] = res[k].T
                for m in range(3):
                    mixed[pp, :, m] = res["mixed"][m].T
            ch ={k: a.reshape(v.d1, v.d2, n, order="F") for k, a in out.items()}
            ch["mixed"] = mixed.reshape(v.d1, v.d2, n, 3, order="F")
            ch["frames"] = fr
            yield ch

    def show_demixed_video(self, path=None, kt=1, frame_range=None, amp_ac=None, range_ac=None, range_Y=None, multi_factor=None, use_craw=False, colors=None):
        """show_demixed_video(obj, save_avi, kt, frame_range, amp_ac, range_ac, range_Y, multi_factor, use_craw)  (@Sources2D/show_demixed_video.m): the six-panel
        video -- raw, background, raw - background, denoised, residual, demixed -- of the displayed frames, every panel mapped to 8 bits by imagesc's rule
        (hostops.imagesc_8bit) in grey within the ranges of :36-57 (hostops.demix_ranges), tiled 2 x 3 in the reference's positions (hostops.demixed_montage).
        path: a multi-page TIFF is written there through PIL, one page per displayed frame (RuntimeError without PIL); None: nothing is written.  Returns the
        ranges (range_ac, range_res, range_Y, multi_factor, amp_ac).
        Deviations: no figure, no titles, no time stamp; a TIFF in place of the AVI; the default range_Y takes the quantiles over ALL samples of the first chunk's raw
        panel (the reference: over 10 000 random samples)."""
        if not self._can("bg_svd_demix"):
            self._svd_refuse("show_demixed_video")
        Image = Tiff = None
        if path is not None:
            try:
                from PIL import Image, TiffImagePlugin as Tiff
            except ImportError as e:
                raise RuntimeError("show_demixed_video(path=...) writes the TIFF through PIL, which is not installed") from e
        amp_ac = self._default_amp_ac(use_craw) if amp_ac is None else float(amp_ac)
        ranges, writer = None, None
        try:
            for ch in self.demixed_frames(kt, frame_range, amp_ac, use_craw, colors):
                if ranges is None:
                    ranges = hostops.demix_ranges(amp_ac, ch["raw"] if range_Y is None else None, range_ac, range_Y, multi_factor)
                    ranges["amp_ac"] = amp_ac
                if path is None:
                    continue
                if writer is None:
                    writer = Tiff.AppendingTiffWriter(path, True)
                for j in range(ch["frames"].size):
                    page = hostops.demixed_montage({k: ch[k][:, :, j] for k in ("raw", "bg", "signal", "denoised", "residual", "mixed")}, ranges)
                    Image.fromarray(page).save(writer, format="TIFF")      # (h x w x 3 uint8: RGB)
                    writer.newFrame()
        finally:
            if writer is not None:
                writer.close()
        return ranges

    # -- known footprints ---------------------------------------------------------------
    def initTemporal(self, frame_range=None, use_parallel=True):
        """@Sources2D/initTemporal.m:89-168,270-292 (ring model): the traces of the footprints obj.A under the background obj.W / obj.b0 (set_W / set_b0, or an
        earlier fit) on the recording that is uploaded -- the second session of an animal, the next temporal batch (initComponents_batch.m:65), a curated A.  No C
        is read.  Per owned patch: the neurons with any weight in the BLOCK (:106-111), Engine.init_temporal[_job] (the rough start, ten plain sweeps, two more
        with deconv_flag's options) and P.Ymean (:152-153); the stitch weighs every patch's rows with AA of the ORIGINAL footprints on its pixels (:160,276-290; one
        all-reduce when sharded); then obj.deconvTemporal() under deconv_flag (:292), else C = C_raw as :290 leaves it.  Sets C, C_raw (and S, P.kernel_pars,
        P.neuron_sn under deconv_flag); the new traces are the engine's bound matrix, so the update_background_parallel that follows uploads no K x T matrix.
        W and b0 stay as they are (:270).  frame_range: the frames that were uploaded, None or (1, T).
        Not built (NotImplementedError): bg_ssub > 1 (the reference's ring branch multiplies W with the full-resolution block), other frame ranges.
        background_model = 'svd' (:180-192,250-262; an engine with supports_bg_svd_init_temporal, else NotImplementedError): per owned patch the neurons with any
        weight in the PATCH (tmp_block = patch_pos, :103-109) and Engine.init_temporal_lowrank -- the footprints and the patch's b (set_bg_svd, or an earlier
        fit) fitted JOINTLY to every frame, f and b0 of the patch replaced (b0 = the pixel mean), then the same sweeps on Y - (b f + b0).  A patch without
        neurons keeps its b, f and b0 (:156-159).  bg_ssub is ignored, as everywhere in this model.  One deviation: a column of b that is identically zero is
        left out of the joint system and its row of f is 0 (the reference divides by a singular matrix).
        What the svd branch serves is a background that was HANDED to this object -- set_bg_svd: the second session of an animal, the next temporal batch -- or the
        zeros of a fresh object.  Once this object's own update_background_parallel has fitted b, f, b0 to the uploaded recording the call keeps the refusal it had
        before the branch was built (NotImplementedError); set_bg_svd(idx, get_b(idx), get_f(idx), get_b0(idx)) says that the fitted b is the one to extract under."""
        self._need_data()
        if self.bg_model == "svd" and not self._can("bg_svd_init_temporal"):
            self._svd_refuse("initTemporal")
        if self.bg_model == "svd" and self._svd_bg_fitted:
            raise NotImplementedError("initTemporal under background_model = 'svd' extracts traces under a background handed in with set_bg_svd; after this object's own "
                                      "update_background_parallel it is not built (hand the fitted factors back with set_bg_svd to extract under them)")
        v, o, eng = self.video, self.options, self.engine
        if self.bg_model == "svd":
            return self._svd_init_temporal(frame_range)
        if self.ssub > 1:
            raise NotImplementedError("initTemporal: bg_ssub > 1 is not built (initTemporal.m:165-166 multiplies W with the full-resolution block)")
        if frame_range is not None and len(frame_range) and (int(frame_range[0]) != 1 or int(frame_range[1]) != v.T):
            raise NotImplementedError("initTemporal works on the frames that were uploaded, [1, %d] (frame_range = [%d, %d])" % (v.T, int(frame_range[0]), int(frame_range[1])))
        K, T = self.A.shape[1], v.T
        if K == 0:
            raise ValueError("initTemporal needs footprints: obj.A has no columns")
        if not self._can("init_temporal"):
            raise NotImplementedError("this engine has no init_temporal")
        dopt = o.deconv_options if o.deconv_flag else None
        sharded = self._sharded
        eng.stitch_begin(K, T)
        batch = len(v.owned) > 1 and self._can("temporal_jobs")
        jobs = []
        for idx in v.owned:
            self.P["Ymean"][idx] = eng.ymean(v.pid[idx])[v.ind_patch[idx]]                           # :152-153
            ind, A_blk = self._slice(self.A, idx, "block")                                           # :106-111
            self._resid_tag.pop(idx, None)
            if ind.size == 0:
                continue                                                                              # :156-159
            if batch:
                jobs.append((eng.init_temporal_job(v.pid[idx], A_blk, 10, 2, dopt), ind))             # :167-168
                continue
            eng.init_temporal(v.pid[idx], A_blk, 10, 2, dopt, want=False)                            # :167-168
            eng.stitch_add(ind)                                                                       # :285-286
        if jobs:
            eng.temporal_jobs_sweep()
            for job, ind in jobs:
                eng.stitch_add_job(job, ind)                                                          # :285-286
        if sharded:
            eng.stitch_allreduce(self.dist)
        self._ymean_full = None
        lazy = (not o.deconv_flag) and self._can("lazy_traces")
        bound_deconv = o.deconv_flag and not sharded and self._can("bound_deconv") and self._can("lazy_traces")
        self.C_raw = eng.stitch_finish(subtract_min=False, want="lazy" if lazy else ("bound" if bound_deconv else True))      # :289-290
        self.C = self.deconvTemporal() if o.deconv_flag else self.C_raw                               # :292
        return self.C

    def _svd_init_temporal(self, frame_range):
        """initTemporal under background_model = 'svd' (initTemporal.m:103-109,150-159,180-192,270-292); the stitch and the deconvTemporal tail are the ring model's"""
        v, o, eng = self.video, self.options, self.engine
        if frame_range is not None and len(frame_range) and (int(frame_range[0]) != 1 or int(frame_range[1]) != v.T):
            raise NotImplementedError("initTemporal works on the frames that were uploaded, [1, %d] (frame_range = [%d, %d])" % (v.T, int(frame_range[0]), int(frame_range[1])))
        K, T = self.A.shape[1], v.T
        if K == 0:
            raise ValueError("initTemporal needs footprints: obj.A has no columns")
        dopt = o.deconv_options if o.deconv_flag else None
        eng.stitch_begin(K, T)
        for idx in v.owned:
            self.P["Ymean"][idx] = eng.ymean(v.pid[idx])[v.ind_patch[idx]]                           # :152-153
            ind = self._slice(self.A, idx, "patch")[0]                                               # :103-109 with tmp_block = patch_pos
            if ind.size == 0:
                continue                                                                              # :156-159: b, f, b0 of this patch stay
            A_blk = self._slice(self.A, idx, "block", cols=ind)[1]                                   # (the engine takes BLOCK rows and drops those outside the patch)
            self._resid_tag.pop(idx, None)
            eng.init_temporal_lowrank(v.pid[idx], A_blk, 10, 2, dopt, want=False)                    # :180-192
            eng.stitch_add(ind)                                                                       # :285-286
        self._ymean_full = None
        lazy = (not o.deconv_flag) and self._can("lazy_traces")
        bound_deconv = o.deconv_flag and self._can("bound_deconv") and self._can("lazy_traces")
        self.C_raw = eng.stitch_finish(subtract_min=False, want="lazy" if lazy else ("bound" if bound_deconv else True))      # :289-290
        self.C = self.deconvTemporal() if o.deconv_flag else self.C_raw                               # :292
        return self.C

    # -- temporal -----------------------------------------------------------------------
    def update_temporal_parallel(self, use_parallel=True, use_c_hat=True):
        """@Sources2D/update_temporal_parallel.m:62-94,112-186,264-295.  The per-patch traces never leave the device: every patch's
        aa .* C_raw is added to the engine's stitch accumulator (:269-278), sharded runs all-reduce that buffer in place (the
        overlap-region stitch, ONE collective), and :279-286 run on the device; one K x T copy comes back for obj.C_raw / obj.C."""
        self._need_data()
        if self.bg_model == "svd":
            return self._svd_update_temporal(use_c_hat)
        v, o, eng = self.video, self.options, self.engine
        K, T = self.C.shape
        launched_any = False
        sharded = self._sharded
        eng.stitch_begin(K, T)
        # several patches on this rank: every patch's update is set up first and the Gauss-Seidel sweeps run level by level ACROSS the patches (they are
        # independent: the reference's parfor, :112-186) -- one patch's level is a few workgroups as long as one trace's work
        batch = use_c_hat and len(v.owned) > 1 and self._can("temporal_jobs")
        jobs = []
        for idx in v.owned:
            pp, bp = v.patch_pix[idx], v.block_pix[idx]
            A_prev_b, C_prev_b = self._prev_block_args(idx)                                          # :90-91
            launched = not launched_any
            whole = bp.size == v.d1 * v.d2                                 # this block is the whole field of view (then so is the patch): no row slicing
            if launched:
                # the sweep (:149-152) only needs (A_prev, C_prev): start it, slice the current A underneath it
                if not self._temporal_residual_done(idx):
                    self._residual(idx, A_prev_b, C_prev_b)
                launched_any = True
                self._cur_blocks, self._cur_blocks_src = {}, self.A
            if whole:
                A_csc = self.A if sp.isspmatrix_csc(self.A) else self.A.tocsc()
                ind = np.nonzero(np.asarray(A_csc.sum(axis=0)).ravel() > 0)[0]                       # :83
                A_pp = A_csc if ind.size == K else A_csc[:, ind]
                self._cur_blocks[idx] = (ind, A_pp)
            else:
                # (ind, A(block, ind)): also what the next background update fits against (update_background_parallel.m:128-130); A(patch, ind) in the same pass
                ind, A_blk, A_pp = self._slice_block_patch(self.A, idx)                              # :83, A_patch(ind_patch,:)
                self._cur_blocks[idx] = (ind, A_blk)
            if ind.size == 0:
                continue                                                                              # :123
            if not launched and not self._temporal_residual_done(idx):
                self._residual(idx, A_prev_b, C_prev_b)          # :149-152
            C_patch = self._rows(self.C, ind)                                                        # :86
            if not use_c_hat:                                                                         # :174-175
                eng.fast_temporal(v.pid[idx], A_pp, want_raw=False)
            elif batch:
                jobs.append((eng.hals_temporal_job(v.pid[idx], A_pp, C_patch, o.maxIter, o.deconv_options if o.deconv_flag else None), ind))
                continue
            elif o.deconv_flag:                                                                       # :106-110
                self._start_wanted_prefetch()
                eng.hals_temporal_deconv(v.pid[idx], A_pp, C_patch, o.maxIter, o.deconv_options, want_all=None)
            else:
                self._start_wanted_prefetch()
                early, self._early_u = self._early_u, None
                if (early is not None and whole and A_pp is early[1] and self.A is early[1] and ind.size == K and not sharded and len(v.owned) == 1
                        and self._can("temporal_early")):
                    eng.temporal_early_claim(early[0])       # (A is exactly the spatial result the projection was queued for: hand-over)
                eng.hals_temporal(v.pid[idx], A_pp, C_patch, o.maxIter, want_C=False, want_raw=False,
                                  **({"want_aa": False} if self._can("temporal_early") else {}))            # :180-181
            eng.stitch_add(ind)                                                                       # :274-275
        if jobs:
            self._start_wanted_prefetch()                                  # host thread under the (GIL-free) sweep / stitch / fit calls that follow
            eng.temporal_jobs_sweep()
            for job, ind in jobs:
                eng.stitch_add_job(job, ind)                                                          # :274-275
        if sharded:                                                        # the overlap-region stitch: ONE all-reduce, in place on the device
            eng.stitch_allreduce(self.dist)
        # without deconvolution nobody needs the values on the host right away: the engine keeps the matrix bound and streams a copy into pinned
        # memory behind the kernels (LazyHostTraces); the next background fit is set up while the temporal sweep is still running
        lazy = (not o.deconv_flag) and self._can("lazy_traces")
        bound_deconv = o.deconv_flag and not sharded and self._can("bound_deconv") and self._can("lazy_traces")
        C_raw = eng.stitch_finish(subtract_min=not o.deconv_flag, want="lazy" if lazy else ("bound" if bound_deconv else True))       # :279-280, :285
        self.C_raw = C_raw
        self.C = self.deconvTemporal() if o.deconv_flag else C_raw        # :282-283 obj.C = obj.deconvTemporal() / :286 (already the engine's bound matrix)
        self._update_b0_new()                                                                         # :291-295
