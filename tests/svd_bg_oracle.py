"""Float64 oracle of background_model = 'svd': a NumPy statement of the arithmetic of endoscope/fit_svd_model.m and svdsecon.m, and of the three update methods
of @Sources2D with that model.  Written from the formulas; nothing of the reference's text is here.

fit_svd_model(Y, nb, A, C, ..., ind_patch) on a block (d_b x T):
    Ymean = mean(Y, 2); Cmean = mean(C, 2); Bf = (Y - Ymean) - A (C - Cmean)               (no A: A = ones(d_b, 1), C = zeros(1, T))
    nb == 0:  b = f = 0,  b0 = Ymean(ind_patch) - A(ind_patch, :) Cmean
    [u, s, v] = svdsecon(Bf - mean(Bf, 2), nb):  the nb leading eigenpairs of the SMALLER Gram (X X' when d_b <= T, else X' X), s = sqrt(|lambda|), the other side X' u / s or X v / s
    b = u(ind_patch, :) s;  f = v';  b0 = Ymean(ind_patch) - A(ind_patch, :) Cmean - b mean(f, 2)
The outlier branch of the reference tests a variable that never exists, so thresh_outlier, sn, b_old and f_old play no part: they are accepted here and ignored."""
import numpy as np
import scipy.sparse as sp

import cnmfe_oracle as orc


def svdsecon(X, k):
    """(U, s, V) with X ~ U diag(s) V', the k leading triplets, from the eigenpairs of the smaller Gram matrix"""
    X = np.asarray(X, dtype=np.float64)
    m, n = X.shape
    assert k <= m and k <= n
    if m <= n:
        w, E = np.linalg.eigh(X @ X.T)
        order = np.argsort(-np.abs(w))[:k]
        U = E[:, order]; s = np.sqrt(np.abs(w[order]))
        V = (X.T @ U) / s
    else:
        w, E = np.linalg.eigh(X.T @ X)
        order = np.argsort(-np.abs(w))[:k]
        V = E[:, order]; s = np.sqrt(np.abs(w[order]))
        U = (X @ V) / s
    return U, s, V


def fit_svd_model(Y, nb, A=None, C=None, b_old=None, f_old=None, thresh_outlier=None, sn=None, ind_patch=None):
    """-> (b (d, nb), f (nb, T), b0 (d,)), d = the pixels ind_patch selects.  b_old, f_old, thresh_outlier, sn: dead arguments (see the module text)."""
    Y = np.asarray(Y, dtype=np.float64)
    d_b, T = Y.shape
    Ymean = Y.mean(axis=1)
    if A is None or A.shape[1] == 0:
        A = np.ones((d_b, 1)); C = np.zeros((1, T))
    A = np.asarray(A.todense()) if sp.issparse(A) else np.asarray(A, dtype=np.float64)
    C = np.asarray(C, dtype=np.float64)
    Cmean = C.mean(axis=1)
    ip = np.ones(d_b, dtype=bool) if ind_patch is None else np.asarray(ind_patch).reshape(-1)
    if nb == 0:
        return np.zeros((int(ip.sum()), 0)), np.zeros((0, T)), Ymean[ip] - A[ip] @ Cmean
    Bf = (Y - Ymean[:, None]) - A @ (C - Cmean[:, None])
    U, s, V = svdsecon(Bf - Bf.mean(axis=1, keepdims=True), nb)
    b = U[ip] * s
    f = V.T
    b0 = Ymean[ip] - A[ip] @ Cmean - b @ f.mean(axis=1)
    return b, f, b0


def singular_values(Y, A=None, C=None):
    """the singular values of the matrix the fit decomposes (for the well-posedness assertions of the cases)"""
    Y = np.asarray(Y, dtype=np.float64)
    Bf = Y - Y.mean(axis=1, keepdims=True)
    if A is not None and A.shape[1]:
        C = np.asarray(C, dtype=np.float64)
        Bf = Bf - (A @ (C - C.mean(axis=1, keepdims=True)))
    return np.linalg.svd(Bf - Bf.mean(axis=1, keepdims=True), compute_uv=False)


class SvdOracleLoop:
    """update_background_parallel / update_spatial_parallel / update_temporal_parallel with background_model = 'svd' (no deconvolution): the background is fitted on the
    BLOCK with the neurons that touch it; both updates select neurons by the PATCH rectangle and work on the patch without halo, Ysig = Y - (b f + b0)."""

    def __init__(self, Yfull, d1, d2, T, patch_dims, w_overlap, A, C, nb=1, spatial_algorithm="hals", maxIter=5, sn=None):
        self.Y = np.asarray(Yfull, dtype=np.float64)
        self.d1, self.d2, self.T, self.nb = d1, d2, T, int(nb)
        self.patch_pos, self.block_pos = orc.distribute_geometry(d1, d2, patch_dims, w_overlap)
        self.A = sp.csc_matrix(A, dtype=np.float64)
        self.C = np.array(C, dtype=np.float64)
        self.C_raw = self.C.copy()
        self.spatial_algorithm, self.maxIter = spatial_algorithm, maxIter
        self.sn = np.ones(d1 * d2) if sn is None else np.asarray(sn, dtype=np.float64).reshape(-1)
        self.b, self.f, self.b0 = {}, {}, {}
        for idx in self._patches():
            n = int(self._mask(self.patch_pos[idx]).sum())
            self.b[idx], self.f[idx], self.b0[idx] = np.zeros((n, self.nb)), np.zeros((self.nb, T)), np.zeros(n)

    def _patches(self):
        nr, nc = self.patch_pos.shape
        return [(m, n) for n in range(nc) for m in range(nr)]

    def _mask(self, pos):
        r0, r1, c0, c1 = [int(v) for v in pos]
        m = np.zeros((self.d1, self.d2), dtype=bool)
        m[r0 - 1:r1, c0 - 1:c1] = True
        return m.reshape(-1, order="F")

    def _data(self, pos):
        r0, r1, c0, c1 = [int(v) for v in pos]
        return self.Y[r0 - 1:r1, c0 - 1:c1, :].reshape(-1, self.T, order="F")

    def ysig(self, idx):
        return self._data(self.patch_pos[idx]) - (self.b[idx] @ self.f[idx] + self.b0[idx][:, None])

    def update_background_parallel(self):
        b1 = self.b[self._patches()[0]]
        flag_first = b1.size == 0 or float(np.mean(b1)) == 0.0
        for idx in self._patches():
            p, b = self.patch_pos[idx], self.block_pos[idx]
            mb = self._mask(b)
            ind = np.nonzero(np.asarray(self.A[mb, :].sum(axis=0)).ravel() > 0)[0]
            if ind.size == 0 and not flag_first:
                continue
            A_block = self.A[mb, :][:, ind]
            self.b[idx], self.f[idx], self.b0[idx] = fit_svd_model(self._data(b), self.nb, A_block if ind.size else None, self.C[ind] if ind.size else None,
                                                                   ind_patch=orc.ind_patch_mask(p, b))

    def update_spatial_parallel(self):
        d1, d2 = self.d1, self.d2
        IND = orc.determine_search_location(self.A, d1, d2)
        K = self.A.shape[1]
        A_ = np.zeros((d1 * d2, K))
        for idx in self._patches():
            mp = self._mask(self.patch_pos[idx])
            ind = np.nonzero(IND[mp, :].any(axis=0))[0]
            if ind.size == 0:
                continue
            A_pp = self.A[mp, :][:, ind]
            IND_patch = IND[mp, :][:, ind]
            Ysig = self.ysig(idx)
            if self.spatial_algorithm == "hals":
                temp = orc.HALS_spatial(Ysig, A_pp, self.C[ind], IND_patch, 3)
            elif self.spatial_algorithm == "hals_thresh":
                temp = orc.HALS_spatial_thresh(Ysig, A_pp, self.C[ind], IND_patch, 3, self.sn[mp])
            else:
                temp = orc.nnls_spatial(Ysig, A_pp, self.C[ind], IND_patch, 20)
            rows = np.nonzero(mp)[0]
            for j, k in enumerate(ind):
                A_[rows, k] = temp[:, j]
        self.A_raw = A_.copy()
        self.A = sp.csc_matrix(orc.post_process_spatial(A_.reshape(d1, d2, K, order="F"), True, False))

    def update_temporal_parallel(self):
        K, T = self.C.shape
        C_new = np.zeros((K, T)); aa = np.zeros(K)
        for idx in self._patches():
            mp = self._mask(self.patch_pos[idx])
            ind = np.nonzero(np.asarray(self.A[mp, :].sum(axis=0)).ravel() > 0)[0]
            if ind.size == 0:
                continue
            A_pp = self.A[mp, :][:, ind]
            _, C_raw_p, _ = orc.HALS_temporal(self.ysig(idx), A_pp, self.C[ind], self.maxIter, None)
            aa_p = np.asarray(A_pp.multiply(A_pp).sum(axis=0)).ravel()
            for j, k in enumerate(ind):
                C_new[k] += C_raw_p[j] * aa_p[j]
                aa[k] += aa_p[j]
        aa[aa == 0] = 1
        self.C_raw = C_new / aa[:, None]
        self.C_raw = self.C_raw - self.C_raw.min(axis=1, keepdims=True)
        self.C = self.C_raw.copy()

    def reconstruct_background(self):
        out = np.zeros((self.d1 * self.d2, self.T))
        for idx in self._patches():
            out[self._mask(self.patch_pos[idx])] = self.b[idx] @ self.f[idx] + self.b0[idx][:, None]
        return out.reshape(self.d1, self.d2, self.T, order="F")
