"""TEST INFRASTRUCTURE: literal float64 NumPy restatements of the three merges and of tag_neurons_parallel,
    @Sources2D/merge_high_corr.m, @Sources2D/merge_neurons_dist_corr.m, @Sources2D/merge_close_neighbors.m, @Sources2D/Sources2D.m:744-759,1683-1715
on plain arrays (A dense or sparse d x K, C / C_raw / S K x T, kernel_pars K), with oracle/oasis_oracle.py's deconvolveCa_ar1_foopsi and GetSn.  The alternation of a
group forms `data` explicitly, as the reference does.  Indices are 0-based.  Nothing here is imported by the product.

Every function also returns its DECISION MARGINS (tests/greedy_oracle.py's idea): for each comparison between a data-derived number and a threshold the smallest
distance seen -- absolute for correlations, overlaps and distances, relative for the tag ratios and the 2 sn cut of the S-less branch."""
import os
import sys

import numpy as np
import scipy.sparse as sp

HERE = os.path.dirname(os.path.abspath(__file__))
for p_ in (os.path.join(os.path.dirname(HERE), "oracle"), HERE):
    if p_ not in sys.path:
        sys.path.insert(0, p_)

import oasis_oracle as oo


class Margins(dict):
    def see(self, key, dist):
        dist = np.asarray(dist, dtype=np.float64)
        dist = dist[np.isfinite(dist)]
        if dist.size:
            self[key] = min(self.get(key, np.inf), float(dist.min()))


def _dense(A):
    return np.asarray(A.todense() if sp.issparse(A) else A, dtype=np.float64)


def corr_rows(X):
    """corr(X'): Pearson's r of the rows; a row without variance gives NaN (0 / 0)"""
    X = np.asarray(X, dtype=np.float64)
    Xc = X - X.mean(axis=1, keepdims=True)
    n = np.sqrt((Xc * Xc).sum(axis=1))
    with np.errstate(divide="ignore", invalid="ignore"):
        return (Xc @ Xc.T) / (n[:, None] * n[None, :])


def connected_components_bruteforce(flag):
    """graph_connected_comp by repeated flooding: labels in the order of each component's lowest node"""
    flag = np.asarray(flag, dtype=bool)
    flag = flag | flag.T
    K = flag.shape[0]
    lab = -np.ones(K, dtype=np.int64)
    c = 0
    for s in range(K):
        if lab[s] >= 0:
            continue
        lab[s] = c
        grew = True
        while grew:
            grew = False
            for i in range(K):
                if lab[i] == c:
                    for j in range(K):
                        if flag[i, j] and lab[j] < 0:
                            lab[j] = c; grew = True
        c += 1
    return lab, c


def groups_of(flag):
    """[l, c] = graph_connected_comp(sparse(flag_merge)); MC = (l == 1:c); MC(:, sum(MC, 1) == 1) = []        (merge_high_corr.m:82-85)"""
    lab, c = connected_components_bruteforce(flag)
    out = [np.flatnonzero(lab == k) for k in range(c)]
    return [g for g in out if g.size > 1]


def diff_spikes(C_raw, mg=None):
    """S_ = diff(C_raw, 1, 2); S_(:, end + 1) = 0; S_(S_ < 2 * GetSn(S_)) = 0      (merge_high_corr.m:59-65, GetSn per row)"""
    C_raw = np.asarray(C_raw, dtype=np.float64)
    S_ = np.zeros_like(C_raw)
    S_[:, :-1] = np.diff(C_raw, axis=1)                                         # :59,63
    for k in range(S_.shape[0]):
        if not np.any(S_[k]):
            continue                                                            # (GetSn of zeros: 0, nothing is below it)
        cut = 2.0 * oo.GetSn(S_[k])
        if mg is not None and cut > 0:
            mg.see("diff_cut", np.abs(S_[k] - cut) / cut)
        S_[k][S_[k] < cut] = 0                                                  # :65
    return S_


def ar2exp1(g):
    """ar2exp(g)(1) for one AR coefficient (ar2exp.m:3-10): roots([1, -g, 0]) = {g, 0}; tau_d = -1 / log(max)"""
    with np.errstate(divide="ignore", invalid="ignore"):
        return -1.0 / np.log(np.maximum(np.asarray(g, dtype=np.float64), 0.0))


def centers(A, d1, d2, method):
    A = _dense(A)
    if str(method).lower() in ("mean", "center"):                               # com.m:20-28
        pix = np.arange(d1 * d2)
        x = pix % d1 + 1.0; y = pix // d1 + 1.0
        with np.errstate(divide="ignore", invalid="ignore"):
            cm = np.stack([x @ A, y @ A], axis=1) / A.sum(axis=0)[:, None]
        cm[cm < 0] = 0; cm[cm[:, 0] > d1, 0] = d1; cm[cm[:, 1] > d2, 1] = d2
        return cm[:, 0], cm[:, 1]
    temp = np.argmax(A, axis=0)                                                 # [~, temp] = max(A_, [], 1)        merge_neurons_dist_corr.m:64
    return temp % d1 + 1.0, temp // d1 + 1.0                                    # ind2sub                            :65


def _decay_flag(kernel_pars, max_decay_diff):
    taud = ar2exp1(kernel_pars)                                                 # merge_high_corr.m:74-78
    with np.errstate(invalid="ignore"):
        return np.abs(taud[:, None] - taud[None, :]) < max_decay_diff           # :79-80


def merge_groups_apply(A, C, C_raw, S, kernel_pars, groups, deconv):
    """merge_high_corr.m:116-236 (the same lines in the other two files): returns dict(A, C, C_raw, S, kernel_pars, keep, merged_ROIs, newIDs, ai, ci)"""
    A = _dense(A).copy(); C = np.array(C, dtype=np.float64); C_raw = np.array(C_raw, dtype=np.float64)
    S = None if S is None else np.array(S, dtype=np.float64)
    kp = np.zeros(C.shape[0]) if kernel_pars is None else np.array(kernel_pars, dtype=np.float64)
    A_, C_raw_ = A.copy(), C_raw.copy()                                         # :23,27 (the copies the loop reads)
    K = C.shape[0]
    ind_del = np.zeros(K, dtype=bool); newIDs = np.zeros(K, dtype=np.int64)
    ais, cis = [], []
    for IDs in groups:
        active = A_[:, IDs].sum(axis=1) > 0                                     # :173
        data = A_[np.ix_(active, IDs)] @ C_raw_[IDs]                            # :176
        ci = C_raw_[IDs[0]].copy()                                              # :177
        for _ in range(10):                                                     # :178-181
            ai = data @ ci / (ci @ ci)
            ci = ai @ data / (ai @ ai)
        A[active, IDs[0]] = ai                                                  # :183
        C_raw[IDs[0]] = ci                                                      # :184
        c, s, b, g = oo.deconvolveCa_ar1_foopsi(ci, oo.GetSn(ci), None, **deconv)      # :187 (options.sn empty: GetSn(y), deconvolveCa.m)
        C[IDs[0]] = c
        if S is not None:
            S[IDs[0]] = s
        kp[IDs[0]] = g                                                          # :188
        newIDs[IDs[0]] = 1                                                      # :189
        ind_del[IDs[1:]] = True                                                 # :191
        ais.append((np.flatnonzero(active), ai)); cis.append(ci)
    keep = np.flatnonzero(~ind_del)
    return dict(A=A[:, keep], C=C[keep], C_raw=C_raw[keep], S=None if S is None else S[keep], kernel_pars=kp[keep], keep=keep,
                merged_ROIs=[np.asarray(g) for g in groups], newIDs=np.flatnonzero(newIDs[keep]), ai=ais, ci=cis)       # :197-198,236


def merge_high_corr(A, C, C_raw, S, kernel_pars, merge_thr, deconv=None):
    """@Sources2D/merge_high_corr.m:41-85 then :116-236.  merge_thr: scalar, [A, C, S] or [A, C, S, max_decay_diff]"""
    mg = Margins()
    thr = np.atleast_1d(np.asarray(merge_thr, dtype=np.float64))
    if thr.size == 1:
        thr = np.array([0.0, thr[0], 0.0])                                      # :41-43
    Ad = _dense(A)
    K = Ad.shape[1]
    with np.errstate(divide="ignore", invalid="ignore"):
        temp = Ad * (1.0 / np.sqrt((Ad ** 2).sum(axis=0)))                      # :52
    A_overlap = temp.T @ temp                                                   # :54
    S_ = S
    if S_ is None or np.asarray(S_).shape[0] != np.asarray(C).shape[0]:         # :57
        S_ = diff_spikes(C_raw, mg)                                             # :58-65
    S_corr = corr_rows(S_) - np.eye(K)                                          # :67
    C_corr = corr_rows(C) - np.eye(K)                                           # :68
    off = ~np.eye(K, dtype=bool)
    # (footprints without a common pixel overlap by exactly 0.0 in any summation order: against the scalar form's A threshold of 0 that is no rounding question)
    mg.see("A_overlap", np.abs(A_overlap - thr[0])[off & ~((A_overlap == 0) & (thr[0] == 0))]); mg.see("C_corr", np.abs(C_corr - thr[1])[off]); mg.see("S_corr", np.abs(S_corr - thr[2])[off])
    with np.errstate(invalid="ignore"):
        flag = (A_overlap >= thr[0]) & (C_corr >= thr[1]) & (S_corr >= thr[2])  # :71
    if thr.size > 3:
        flag &= _decay_flag(kernel_pars, thr[3])                                # :72-81
    out = merge_groups_apply(A, C, C_raw, S, kernel_pars, groups_of(flag), deconv or {})
    out["margins"] = mg; out["flag"] = flag
    return out


def merge_neurons_dist_corr(A, C, C_raw, S, kernel_pars, d1, d2, merge_thr, dmin, method_dist="max", max_decay_diff=None, deconv=None):
    """@Sources2D/merge_neurons_dist_corr.m:58-86 then :124-243"""
    mg = Margins()
    K = np.asarray(C).shape[0]
    yy, xx = centers(A, d1, d2, method_dist)                                    # :58-66
    dist_v = np.sqrt((xx[:, None] - xx[None, :]) ** 2 + (yy[:, None] - yy[None, :]) ** 2)      # :67
    C_corr = corr_rows(C) - np.eye(K)                                           # :70
    off = ~np.eye(K, dtype=bool)
    mg.see("dist", np.abs(dist_v - dmin)[off]); mg.see("C_corr", np.abs(C_corr - merge_thr)[off])
    with np.errstate(invalid="ignore"):
        flag = (dist_v <= dmin) & (C_corr >= merge_thr)                         # :73
    if max_decay_diff is not None:
        flag &= _decay_flag(kernel_pars, max_decay_diff)                        # :74-82
    out = merge_groups_apply(A, C, C_raw, S, kernel_pars, groups_of(flag), deconv or {})
    out["margins"] = mg; out["flag"] = flag
    return out


def merge_close_neighbors(A, C, C_raw, S, kernel_pars, d1, d2, dmin, method_dist="max", deconv=None):
    """@Sources2D/merge_close_neighbors.m:49-83 then :120-237"""
    mg = Margins()
    dmin = np.atleast_1d(np.asarray(dmin, dtype=np.float64))
    K = np.asarray(C).shape[0]
    yy, xx = centers(A, d1, d2, method_dist)                                    # :49-57
    dist_v = np.sqrt((xx[:, None] - xx[None, :]) ** 2 + (yy[:, None] - yy[None, :]) ** 2)      # :58
    mg.see("dist", np.abs(dist_v - dmin[0])[~np.eye(K, dtype=bool)])
    flag = dist_v <= dmin[0]                                                    # :62
    if dmin.size > 1:
        flag &= _decay_flag(kernel_pars, dmin[1])                               # :66-79
    out = merge_groups_apply(A, C, C_raw, S, kernel_pars, groups_of(flag), deconv or {})
    out["margins"] = mg; out["flag"] = flag
    return out


def tag_neurons(A, C, C_raw, S, min_pixel, deconv_flag=True, min_pnr=3.0):
    """tag_neurons_parallel (Sources2D.m:1683-1715).  Returns (tags uint16, margins)"""
    mg = Margins()
    Ad = _dense(A)
    nz_pixels = (Ad > 0).sum(axis=0)                                            # :1695
    tags = (nz_pixels < min_pixel).astype(np.uint16)                            # :1696
    if deconv_flag:
        C = np.asarray(C, dtype=np.float64); C_raw = np.asarray(C_raw, dtype=np.float64); S = np.asarray(S, dtype=np.float64)
        nz_spikes = (S[:, 1:] > 0).sum(axis=1)                                  # :1700
        tags += (nz_spikes < 1).astype(np.uint16) * 2                           # :1701
        tmp_std = np.std(C_raw - C, axis=1, ddof=1)                             # :1703
        sn = np.array([oo.GetSn(r) for r in C_raw])
        with np.errstate(divide="ignore", invalid="ignore"):
            temp = tmp_std / sn                                                 # :1705
            pnrs = C.max(axis=1) / tmp_std                                      # :1709
            mg.see("noise_ratio", np.abs(temp - 0.1) / 0.1); mg.see("pnr", np.abs(pnrs - min_pnr) / min_pnr)
            tags += (temp < 0.1).astype(np.uint16) * 4                          # :1706
            tags += (pnrs < min_pnr).astype(np.uint16) * 8                      # :1710
    return tags, mg


def remove_false_positives(A, C, C_raw, S, kernel_pars, min_pixel, deconv_flag=True):
    """Sources2D.m:744-759 -> obj.delete(ids): returns (ids, dict of the kept arrays)"""
    tags, _ = tag_neurons(A, C, C_raw, S, min_pixel, deconv_flag)
    ids = np.flatnonzero(tags)                                                  # :749
    keep = np.setdiff1d(np.arange(len(tags)), ids)
    Ad = _dense(A)
    return ids, dict(A=Ad[:, keep], C=np.asarray(C)[keep], C_raw=np.asarray(C_raw)[keep], S=None if S is None else np.asarray(S)[keep],
                     kernel_pars=None if kernel_pars is None else np.asarray(kernel_pars)[keep], keep=keep)
