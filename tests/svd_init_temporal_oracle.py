"""Float64 restatement of @Sources2D/initTemporal.m under background_model = 'svd' (:103-109, :150-159, :180-192, :270-292): per patch the footprints and the
background's spatial factors are fitted JOINTLY to every frame, f and b0 are replaced, and HALS_temporal's sweeps run on Ypatch - (b f + b0) from that start.
The sweeps, the deconvolution branch and the geometry are those of tests/init_temporal_oracle.py (by import).

One deviation from the reference, shared with the engine: a column of b that is identically zero is left out of the joint system and its row of f is 0
(tmp_A'*tmp_A is singular there and MATLAB's backslash returns Inf / NaN with a warning)."""
import numpy as np
import scipy.sparse as sp

import init_temporal_oracle as ito

orc = ito.orc


def joint_system(Y_patch, A_patch, b, b0=None):
    """(G, R, keep, b0): G = M'M, R = M'(Y - b0 1'), M = [A_patch, b(:, keep)], keep = the columns of b that are not identically zero, b0 = mean(Y, 2)  (:180-182).
    b0 given: that vector instead of the mean (stored_video, below: the mean of the recording, where Y is the engine's stored copy of it)"""
    Y = np.asarray(Y_patch, dtype=np.float64)
    A = ito._dense(A_patch)
    b = np.asarray(b, dtype=np.float64).reshape(Y.shape[0], -1)
    keep = np.any(b != 0, axis=0)
    b0 = Y.mean(axis=1) if b0 is None else np.asarray(b0, dtype=np.float64)      # :180
    M = np.hstack([A, b[:, keep]])                            # :181
    return M.T @ M, M.T @ (Y - b0[:, None]), keep, b0


def cholesky_pivots(G):
    """the pivots (before the square root) of the Cholesky factorisation of G, in order; stops at the first one that is not positive"""
    n = G.shape[0]
    L = np.zeros_like(G)
    piv = []
    for i in range(n):
        for j in range(i + 1):
            s = G[i, j] - L[i, :j] @ L[j, :j]
            if j < i:
                L[i, j] = s / L[j, j]
            else:
                piv.append(s)
                if not s > 0:
                    return np.asarray(piv)
                L[i, i] = np.sqrt(s)
    return np.asarray(piv)


def refusal_threshold(G):
    """a pivot at or below this fails the engine's call: n eps max(diag G)"""
    return G.shape[0] * np.finfo(np.float64).eps * float(np.max(np.diag(G)))


def stored_video(Y_patch32):
    """(Y, b0) of a float32 recording as an engine that keeps the video CENTRED IN FLOAT32 sees it: b0 = the float64 pixel mean, Y = fl32(Y - fl32(b0)) + fl32(b0).
    Where a sample is more than a factor 2 away from its pixel's mean the float32 subtraction rounds (2^-24 relative): an input perturbation no arithmetic behind
    it can undo.  The fit of f averages it over the pixels of a patch; it is what separates an fp64 engine from this oracle on the recording itself."""
    Y32 = np.asarray(Y_patch32, dtype=np.float32)
    b0 = Y32.astype(np.float64).mean(axis=1)
    m32 = b0.astype(np.float32)
    return (Y32 - m32[:, None]).astype(np.float64) + m32.astype(np.float64)[:, None], b0


def init_temporal_patch(Y_patch, A_patch, b, deconv=None, iters=(10, 2), b0=None):
    """initTemporal.m:180-192 of one patch.  Y_patch d x T (the PATCH, no halo), A_patch d x k (the neurons with weight in the patch), b d x nb.
    Returns dict(C, C_raw, S, sn, kernel_pars, AA, C0, f, b0, G, Ysig)."""
    Y = np.asarray(Y_patch, dtype=np.float64)
    A = ito._dense(A_patch)
    b = np.asarray(b, dtype=np.float64).reshape(Y.shape[0], -1)
    k, T = A.shape[1], Y.shape[1]
    G, R, keep, b0 = joint_system(Y, A, b, b0)
    X = np.linalg.solve(G, R)                                 # :182
    C0 = X[:k]                                                # :183
    f = np.zeros((b.shape[1], T)); f[keep] = X[k:]            # :184
    Ysig = Y - (b @ f + b0[:, None])                          # :186
    AA = (A ** 2).sum(axis=0)                                 # :160 (the patch rows)
    C, _, _ = orc.HALS_temporal(Ysig, A, C0, iters[0])        # :191
    out = dict(AA=AA, C0=C0, f=f, b0=b0, G=G, Ysig=Ysig, S=None, sn=None, kernel_pars=None)
    if deconv is None:
        out["C"], out["C_raw"], _ = orc.HALS_temporal(Ysig, A, C, iters[1])                          # :192, deconv_options = []
    else:
        import oasis_oracle as oo
        Cd, Craw, S, sn, kp = oo.HALS_temporal_deconv(Ysig, A, C, iters[1], **deconv)              # :192
        out.update(C=Cd, C_raw=Craw, S=S, sn=sn, kernel_pars=np.array([0.0 if g is None else g for g in kp]))
    return out


def init_temporal(Y_td, A, b, d1, d2, patch_dims, halo, deconv=None):
    """the whole method: Y_td (T, d) frame-major, A d x K, b {(m, n): d_patch x nb}.  Returns dict(C_raw, C, S, kernel_pars, neuron_sn, per_patch, ind, f, b0):
    f / b0 per patch -- None where the patch has no neuron and keeps what it had (:156-159).  C_raw is the AA-weighted stitch (:276-290); with deconv,
    deconvTemporal follows (:292), else C = C_raw."""
    Y = np.asarray(Y_td, dtype=np.float64).T
    A = sp.csc_matrix(A).astype(np.float64)
    K, T = A.shape[1], Y.shape[1]
    patch_pos, _ = orc.distribute_geometry(d1, d2, patch_dims, halo)
    C_new = np.zeros((K, T)); aa = np.zeros(K)
    per_patch, inds, fs, b0s = {}, {}, {}, {}
    for n in range(patch_pos.shape[1]):
        for m in range(patch_pos.shape[0]):
            pp = ito.block_pixels(patch_pos[m, n], d1)                                               # tmp_block = patch_pos (:103)
            A_p = A[pp]
            ind = np.nonzero(np.asarray(A_p.sum(axis=0)).ravel() > 0)[0]                            # :108
            inds[(m, n)] = ind
            fs[(m, n)] = b0s[(m, n)] = None
            if ind.size == 0:
                continue                                                                              # :156-159
            res = init_temporal_patch(Y[pp], A_p[:, ind], b[(m, n)], deconv)
            per_patch[(m, n)] = res
            fs[(m, n)], b0s[(m, n)] = res["f"], res["b0"]
            C_new[ind] += res["C_raw"] * res["AA"][:, None]                                          # :285
            aa[ind] += res["AA"]                                                                      # :286
    aa[aa == 0] = 1                                                                                   # :289
    C_raw = C_new / aa[:, None]                                                                       # :290
    out = dict(C_raw=C_raw, C=C_raw, S=None, kernel_pars=None, neuron_sn=None, per_patch=per_patch, ind=inds, f=fs, b0=b0s)
    if deconv is not None:
        import oasis_oracle as oo
        Cd, Craw, S, kp, sn = oo.deconvTemporal(C_raw, **deconv)                                     # :292
        out.update(C=Cd, C_raw=Craw, S=S, kernel_pars=kp, neuron_sn=sn)
    return out


def sweep_min_margins(Ysig, A, C0, iters):
    """HALS_temporal's plain sweeps (HALS_temporal.m:59-68) once more, recording for every row update how clearly its minimum (:66) is decided: (second smallest -
    smallest) / (largest - smallest) of ck_raw.  Returns (margins, C): C equals orc.HALS_temporal(Ysig, A, C0, iters)[0] bit for bit."""
    Y = np.asarray(Ysig, dtype=np.float64)
    A = ito._dense(A)
    C = np.array(C0, dtype=np.float64, copy=True)
    U = A.T @ Y; V = A.T @ A
    aa = np.diag(V).copy()
    out = []
    for _ in range(iters):
        for k in np.nonzero(aa > 0)[0]:
            ck = C[k, :] + (U[k, :] - V[k, :] @ C) / aa[k]
            s = np.partition(ck, 1)[:2]
            out.append((s[1] - s[0]) / (ck.max() - s[0]))
            C[k, :] = ck - ck.min()
    return np.asarray(out), C
