"""Float64 restatement of @Sources2D/initTemporal.m (ring branch: :89-168, :270-292) on top of oracle/cnmfe_oracle.py (HALS_temporal, the ring
builder, the patch geometry) and oracle/oasis_oracle.py (the deconvolution branch, deconvTemporal).  The rough start of
utilities/HALS_temporal.m:34-41 is written here: the committed oracle's HALS_temporal requires a C."""
import numpy as np
import scipy.sparse as sp

import cnmfe_oracle as orc


def _dense(A):
    return np.asarray(A.toarray() if sp.issparse(A) else A, dtype=np.float64)


def rough_start(Y, A):
    """HALS_temporal.m:34-41 (C is empty).  Returns (C0, tmp_A, tmpA): the start, the selection A .* ind_max and the column-normalised A the
    winners are read from."""
    Y = np.asarray(Y, dtype=np.float64)
    A = _dense(A)
    with np.errstate(divide="ignore", invalid="ignore"):
        tmpA = A * (1.0 / A.sum(axis=0))[None, :]            # :36  bsxfun(@times, A, 1./sum(A, 1))
        mx = np.fmax.reduce(tmpA, axis=1)                    # :37  max(tmpA, [], 2): over ALL K columns, NaN ignored (all-NaN row: NaN)
        ind_max = tmpA == mx[:, None]                        # :37  eq: false against NaN
    tmp_A = A * ind_max                                      # :38
    temp = (tmp_A ** 2).sum(axis=0)                          # :39
    temp[temp == 0] = 1                                      # :40
    C0 = (tmp_A.T @ Y) / temp[:, None]                       # :41
    return C0, tmp_A, tmpA


def winner_margins(tmpA):
    """per pixel with a non-zero entry whose row maximum is a non-zero entry: (top - runner-up) / |top|, the runner-up taken over all other columns
    (zeros compete).  What a fixture must keep away from 0 so that no implementation can differ from this oracle in a discrete choice."""
    t = np.where(np.isnan(tmpA), -np.inf, tmpA)
    out = []
    for row in t:
        if not np.any(row != 0) or row.size < 2:
            continue
        s = np.sort(row)[::-1]
        if s[0] != 0 and np.isfinite(s[0]):
            out.append((s[0] - s[1]) / abs(s[0]))
    return np.asarray(out)


def init_temporal_patch(Y_block, A_block, W, ind_patch, deconv=None, iters=(10, 2)):
    """initTemporal.m:160-168 of one patch.  Y_block d_b x T, A_block d_b x K (the neurons with weight in the block), W d x d_b, ind_patch the patch rows
    among the block rows.  deconv: None, or the keyword options of oasis_oracle.HALS_temporal_deconv."""
    Y = np.asarray(Y_block, dtype=np.float64)
    A = _dense(A_block)
    W = sp.csr_matrix(W).astype(np.float64)
    ip = np.asarray(ind_patch, dtype=bool).ravel()
    AA = (A[ip] ** 2).sum(axis=0)                            # :160
    Yt = Y[ip] - W @ Y                                       # :165
    At = A[ip] - W @ A                                       # :166
    C0, tmp_A, tmpA = rough_start(Yt, At)
    C, _, _ = orc.HALS_temporal(Yt, At, C0, iters[0])        # :167
    out = dict(AA=AA, At=At, Yt=Yt, C0=C0, tmpA=tmpA, S=None, sn=None, kernel_pars=None)
    if deconv is None:
        out["C"], out["C_raw"], _ = orc.HALS_temporal(Yt, At, C, iters[1])                           # :168, deconv_options = []
    else:
        import oasis_oracle as oo
        Cd, Craw, S, sn, kp = oo.HALS_temporal_deconv(Yt, At, C, iters[1], **deconv)               # :168
        out.update(C=Cd, C_raw=Craw, S=S, sn=sn, kernel_pars=np.array([0.0 if g is None else g for g in kp]))
    return out


def block_pixels(rect, d1):
    r0, r1, c0, c1 = [int(x) for x in rect]
    cc, rr = np.meshgrid(np.arange(c0 - 1, c1), np.arange(r0 - 1, r1))
    return (cc * d1 + rr).reshape(-1, order="F")


def init_temporal(Y_td, A, W, d1, d2, patch_dims, radius, deconv=None, shift=None):
    """the whole method: Y_td (T, d) frame-major, A d x K, W {(m, n): d_patch x d_block}.  Returns dict(C_raw, C, S, kernel_pars, neuron_sn, per_patch, ind).
    C_raw is the AA-weighted stitch (:276-290); with deconv, deconvTemporal follows (:292), else C = C_raw.  shift: a d-vector subtracted from every pixel's
    trace first (the shift-invariance check)."""
    Y = np.asarray(Y_td, dtype=np.float64).T
    if shift is not None:
        Y = Y - np.asarray(shift, dtype=np.float64)[:, None]
    A = sp.csc_matrix(A).astype(np.float64)
    K, T = A.shape[1], Y.shape[1]
    patch_pos, block_pos = orc.distribute_geometry(d1, d2, patch_dims, radius)
    C_new = np.zeros((K, T)); aa = np.zeros(K)
    per_patch, inds = {}, {}
    for n in range(patch_pos.shape[1]):
        for m in range(patch_pos.shape[0]):
            bp = block_pixels(block_pos[m, n], d1)
            ip = orc.ind_patch_mask(patch_pos[m, n], block_pos[m, n])
            A_b = A[bp]
            ind = np.nonzero(np.asarray(A_b.sum(axis=0)).ravel() > 0)[0]                            # :108
            inds[(m, n)] = ind
            if ind.size == 0:
                continue                                                                              # :156-159
            res = init_temporal_patch(Y[bp], A_b[:, ind], W[(m, n)], ip, deconv)
            per_patch[(m, n)] = res
            C_new[ind] += res["C_raw"] * res["AA"][:, None]                                          # :285
            aa[ind] += res["AA"]                                                                      # :286
    aa[aa == 0] = 1                                                                                   # :289
    C_raw = C_new / aa[:, None]                                                                       # :290
    out = dict(C_raw=C_raw, C=C_raw, S=None, kernel_pars=None, neuron_sn=None, per_patch=per_patch, ind=inds)
    if deconv is not None:
        import oasis_oracle as oo
        Cd, Craw, S, kp, sn = oo.deconvTemporal(C_raw, **deconv)                                     # :292
        out.update(C=Cd, C_raw=Craw, S=S, kernel_pars=kp, neuron_sn=sn)
    return out
