"""TEST INFRASTRUCTURE: float64 NumPy restatement of the greedy initialisation of one block and of the collection over the patches,
    @Sources2D/initComponents_parallel.m:200-203,308-352,410-484 -> endoscope/greedyROI_endoscope.m:62-164,193-216,262-311,339-410,447-463
    -> endoscope/extract_ac.m, endoscope/remove_baseline.m, OASIS_matlab/functions/estimate_baseline_noise.m, fit_gauss1.m
from the RAW video as the reference sees it.  Built on tests/seed_oracle.py (filter, detrending, correlation image), oracle/cnmfe_oracle.py (constraints,
_medfilt3, matlab_quantile) and oracle/oasis_oracle.py (GetSn, deconvolution).  Nothing here is imported by the product.

Besides the results every run returns its DECISION MARGINS: for each comparison the algorithm makes between a data-derived number and a threshold (or another
data-derived number) the smallest distance seen.  A fixture whose margins are wide enough pins every discrete decision of the run, whatever the rounding of
an fp32 implementation (tests/test_greedy_oracle.py checks the fixtures, tests/test_gpu_init.py relies on it)."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
for p_ in (os.path.join(os.path.dirname(HERE), "oracle"), HERE):
    if p_ not in sys.path:
        sys.path.insert(0, p_)

import cnmfe_oracle as orc
import oasis_oracle as oo
import seed_oracle as so


class Margins(dict):
    """key -> the smallest distance seen.  corr, cn: absolute; everything else relative to the threshold"""
    def see(self, key, dist):
        dist = np.asarray(dist, dtype=np.float64)
        dist = dist[np.isfinite(dist)]
        if dist.size:
            self[key] = min(self.get(key, np.inf), float(dist.min()))


# ---- single-trace functions -------------------------------------------------------------------------------------------------------------------------------
def hist_centres(y, centres):
    """hist(y, centres): one bin per centre, the edges half-way between neighbouring centres, the outer bins open; a value on an edge counts below it"""
    nums = np.zeros(len(centres))
    for v in np.asarray(y, dtype=np.float64).ravel():
        k = 0
        while k < len(centres) - 1 and v > 0.5 * (centres[k] + centres[k + 1]):
            k += 1
        nums[k] += 1
    return nums


def fit_gauss1(x, y, thr=0.1, maxIter=5, mu_fix=False):
    """fit_gauss1.m:21-87 with lstsq-free normal equations written out as in the reference"""
    x = np.asarray(x, dtype=np.float64).ravel(); y = np.asarray(y, dtype=np.float64).ravel()
    ind = y > y.max() * thr
    x = x[ind]; y = y[ind]
    logy = np.log(y)
    p = None
    with np.errstate(all="ignore"):
        for _ in range(maxIter):
            w = y ** 2
            cols = [np.ones_like(x), x ** 2] if mu_fix else [np.ones_like(x), x, x ** 2]
            M = np.array([[np.sum(ci * cj * w) for cj in cols] for ci in cols])
            b = np.array([np.sum(ci * w * logy) for ci in cols])
            try:
                p = np.linalg.solve(M, b)
            except np.linalg.LinAlgError:
                p = np.full(len(cols), np.nan)
            logy = sum(pk * ck for pk, ck in zip(p, cols))
            y = np.exp(logy)
    if mu_fix:
        return 0.0, float(np.sqrt(-0.5 / p[1])), float(np.exp(p[0]))
    return float(-p[1] / 2 / p[2]), float(abs(np.sqrt(complex(-0.5 / p[2])))), float(np.exp(p[0] - 0.25 * p[1] ** 2 / p[2]))


def estimate_baseline_noise(y):
    """estimate_baseline_noise.m:18-29 (bmin = -Inf)"""
    y = np.asarray(y, dtype=np.float64).ravel()
    temp = np.array([orc.matlab_quantile(y, q / 10.0) for q in range(11)], dtype=np.float64).ravel()
    dbin = max(np.min(np.diff(temp)) / 3.0, (temp.max() - temp.min()) / 1000.0)
    if not dbin > 0:
        return float(y.mean()), 0.0
    nb = int(np.floor((temp[-1] - temp[0]) / dbin + 1e-10)) + 1
    bins = temp[0] + dbin * np.arange(nb)
    b, sn, _ = fit_gauss1(bins, hist_centres(y, bins), 0.3, 3)
    return b, sn


def remove_baseline(y, sn):
    y = np.asarray(y, dtype=np.float64)
    dy = np.concatenate([[-1.0], y[1:] - y[:-1]])
    sel = np.sort(y[(dy >= 0) & (dy < sn)])
    b = np.nan if sel.size == 0 else 0.5 * (sel[(sel.size - 1) // 2] + sel[sel.size // 2])
    return y - b, b


def window_max_brute(v, n):
    """ordfilt2(v, n^2, true(n)) by its definition: per pixel the maximum over the n x n domain centred at floor((n + 1) / 2) (1-based), zeros outside"""
    nr, nc = v.shape
    c0 = (n + 1) // 2 - 1
    out = np.zeros_like(v, dtype=np.float64)
    for r in range(nr):
        for c in range(nc):
            m = -np.inf
            for i in range(n):
                for j in range(n):
                    rr, cc = r + i - c0, c + j - c0
                    m = max(m, v[rr, cc] if 0 <= rr < nr and 0 <= cc < nc else 0.0)
            out[r, c] = m
    return out


def _box(nr, nc, r, c, reach):
    return max(0, r - reach), min(nr, r + reach + 1), max(0, c - reach), min(nc, c + reach + 1)


def _box_pixels(nr, r0, r1, c0, c1):
    cc, rr = np.meshgrid(np.arange(c0, c1), np.arange(r0, r1), indexing="ij")     # column-major inside the box
    return (cc * nr + rr).ravel()


def pearson_rows(y0, X):
    y = y0 - y0.mean()
    Z = X - X.mean(axis=1, keepdims=True)
    with np.errstate(invalid="ignore", divide="ignore"):
        return (Z @ y) / np.sqrt((Z * Z).sum(axis=1) * (y @ y))


# ---- one block ----------------------------------------------------------------------------------------------------------------------------------------------
def greedy_block(Yb, nr, nc, gSig, gSiz, center_psf=True, nk=1, min_corr=0.3, min_pnr=10.0, min_pixel=5.0, bd4=(0, 0, 0, 0), K=None, connected=True,
                 deconv_opts=None, seeds=None, sig=3.0):
    """greedyROI_endoscope on a block Yb (d_b x T raw video, pixels column-major in nr x nc).  seeds: 0-based block pixels, tried once in the given order
    under the halved thresholds of seed_method 'manual'.  Returns dict(A: list of (box, ai image), C, C_raw, S, kernel_pars, center (1-based), Cn, PNR (the
    initial images), steps (the extract / apply record), margins)."""
    gSiz = int(gSiz)
    mg = Margins()
    Y = np.array(Yb, dtype=np.float64)
    T = Y.shape[1]
    if nk > 1:
        Y = so.detrend_spline(Y, nk)                                       # initComponents_parallel.m:341-343
    psf = so.make_psf(gSig, gSiz, center_psf)
    Y3 = Y.reshape(nr, nc, T, order="F")
    HY = (so.imfilter_replicate(Y3, psf) if psf is not None else Y3.copy()).reshape(nr * nc, T, order="F")
    HY = HY - np.median(HY, axis=1, keepdims=True)                         # :130
    with np.errstate(invalid="ignore", divide="ignore"):
        Sn = np.array([oo.GetSn(row) for row in HY])                       # :132
        PNR0 = (HY.max(axis=1) / Sn).reshape(nr, nc, order="F")
    Cn0 = so.correlation_image(np.where(HY < sig * Sn[:, None], 0.0, HY), nr, nc)
    min_v_search = min_corr * min_pnr
    if seeds is not None:
        min_corr, min_pnr = min_corr / 2.0, min_pnr / 2.0
    PNR = PNR0.copy(); Cn = Cn0.copy()
    with np.errstate(invalid="ignore"):
        mg.see("pnr", np.abs(PNR - min_pnr) / min_pnr); mg.see("cn", np.abs(Cn - min_corr))
        PNR[PNR < min_pnr] = 0
        Cn[np.isnan(Cn)] = 0
        v_search = Cn * PNR
        v_search[(Cn < min_corr) | (PNR < min_pnr)] = 0
    v_search[~np.isfinite(v_search)] = 0
    ind_search = v_search == 0
    ind_bd = np.zeros((nr, nc), dtype=bool)
    if bd4[0] > 0: ind_bd[:bd4[0]] = True
    if bd4[1] > 0: ind_bd[nr - bd4[1]:] = True
    if bd4[2] > 0: ind_bd[:, :bd4[2]] = True
    if bd4[3] > 0: ind_bd[:, nc - bd4[3]:] = True
    nseed = int((v_search > 0).sum()) // 10
    K = nseed if K is None else min(nseed, int(K))
    pixel_v = np.array([[((c + 1) * 10 + (r + 1)) * 1e-10 for c in range(nc)] for r in range(nr)])
    tmp_d = max(3, so.matlab_round(gSiz / 4.0))
    res = dict(A=[], C=[], C_raw=[], S=[], kernel_pars=[], center=[], steps=[])
    k = 0
    searching = True
    while searching and K > 0:
        v_search = orc._medfilt3(v_search) + pixel_v
        v_search[ind_search] = 0
        v_max = window_max_brute(v_search, tmp_d)
        v_search[ind_bd] = 0
        if seeds is not None:
            loc = []
            for (r, c) in seeds:
                if not (0 <= r < nr and 0 <= c < nc) or v_search[r, c] == 0:
                    break
                loc.append((r, c))
            searching = False
        else:
            pos = v_search[v_search > 0]
            mg.see("v_search", np.abs(pos - min_v_search) / min_v_search)
            ind_search[v_search < min_v_search] = True
            cand = [(v_search[r, c], c * nr + r) for c in range(nc) for r in range(nr) if v_search[r, c] == v_max[r, c] and v_max[r, c] > 0]
            cand.sort(key=lambda t: -t[0])                                 # (stable: ties stay in find() order)
            vals = np.array([t[0] for t in cand])
            if vals.size > 1:
                mg.see("localmax", (vals[:-1] - vals[1:]) / vals[:-1])
            loc = [(p % nr, p // nr) for _, p in cand]
        if not loc:
            break
        for (r, c) in loc:
            max_v = v_search[r, c]
            ind_search[r, c] = True
            if max_v > 0:
                mg.see("v_search", abs(max_v - min_v_search) / min_v_search)
            if max_v < min_v_search:
                continue
            p0 = c * nr + r
            y0 = HY[p0]
            dy = np.diff(y0)
            mg.see("diff", abs(dy.max() - 3 * dy.std(ddof=1)) / (3 * dy.std(ddof=1)))
            if dy.max() < 3 * dy.std(ddof=1):
                continue
            r0, r1, c0, c1 = _box(nr, nc, r, c, gSiz)
            s0, s1, t0, t1 = _box(nr, nc, r, c, 2 * gSiz)
            ind = _box_pixels(nr, r0, r1, c0, c1); ind2 = _box_pixels(nr, s0, s1, t0, t1)
            sh, sh2 = (r1 - r0, c1 - c0), (s1 - s0, t1 - t0)
            # ---- extract_ac.m
            HYb, Yw = HY[ind], Y[ind]
            corr = pearson_rows(y0, HYb)
            mg.see("corr", np.minimum(np.abs(corr - 0.9), np.abs(corr - 0.3)))
            with np.errstate(invalid="ignore"):
                hi, lo = corr > 0.9, corr < 0.3
            step = dict(kind="extract", r=r, c=c, hi=hi.reshape(sh, order="F"), lo=lo.reshape(sh, order="F"), ci=None, ai=None)
            res["steps"].append(step)
            ci = HYb[hi].mean(axis=0) if hi.any() else np.full(T, np.nan)
            step["ci"] = ci
            ok = bool(np.isfinite(ci).all() and np.linalg.norm(ci) != 0 and lo.any())
            ai = None
            if ok:
                y_bg = np.median(Yw[lo], axis=0)
                X = np.stack([np.ones(T), y_bg, ci], axis=1)
                temp = np.linalg.lstsq(X, Yw.T, rcond=None)[0]             # (X'X) \ (X'Y')
                ai0 = np.maximum(0.0, temp[2]).reshape(sh, order="F")
                step["ai"] = ai0
                ai = orc.circular_constraints(ai0)
                if connected:
                    ai = orc.connectivity_constraint(ai)
                if (ai > 0).sum() < 5:
                    ok = False
            if ok:
                b, sn = estimate_baseline_noise(ci)
                psd_sn = oo.GetSn(ci)
                mg.see("sn", abs(sn - psd_sn) / psd_sn)
                ci = remove_baseline(ci, psd_sn)[0] if sn > psd_sn else ci - b
                ok = bool(np.linalg.norm(ai) != 0) and not (np.isnan(ai).any() or np.isnan(ci).any())
            if ok:
                mg.see("sum_ai", abs(ai.sum() - min_pixel) / min_pixel)
                mg.see("nnz_ai", abs((ai > 0).sum() - (min_pixel - 0.5)) / min_pixel)
                if ai.sum() <= min_pixel or (ai > 0).sum() < min_pixel:
                    ok = False
            if not ok:
                continue
            k += 1
            ci_raw = ci
            if deconv_opts is not None:
                c_, r_, s_, kp_, _ = oo.deconvTemporal(ci_raw[None, :], **deconv_opts)
                ci, ci_keep, si, pars = c_[0], r_[0], s_[0], float(kp_[0])
            else:
                ci_keep, si, pars = ci_raw, None, None
            res["A"].append(((r0, r1, c0, c1), ai)); res["C"].append(ci); res["C_raw"].append(ci_keep); res["S"].append(si); res["kernel_pars"].append(pars)
            res["center"].append((r + 1, c + 1))
            tmp = ind_search.reshape(-1, order="F"); tmp[ind[(ai > ai.max() * 0.5).reshape(-1, order="F")]] = True
            ind_search = tmp.reshape(nr, nc, order="F")
            Y[ind] = Yw - np.outer(ai.reshape(-1, order="F"), ci)
            big = np.zeros(sh2)
            big[r0 - s0:r1 - s0, c0 - t0:c1 - t0] = ai
            Hai = so.imfilter_replicate(big[:, :, None], psf)[:, :, 0] if psf is not None else big
            HY2 = HY[ind2] - np.outer(Hai.reshape(-1, order="F"), ci)
            HY[ind2] = HY2
            Sn2 = Sn[ind2]
            with np.errstate(invalid="ignore", divide="ignore"):
                pnr2 = HY2.max(axis=1) / Sn2
                mg.see("pnr", np.abs(pnr2 - min_pnr) / min_pnr)
                mg.see("hy", np.abs(HY2 - sig * Sn2[:, None]).min(axis=1) / Sn2)
                pnr2[np.isnan(pnr2) | (pnr2 < min_pnr)] = 0
                cn2 = so.correlation_image(np.where(HY2 < sig * Sn2[:, None], 0.0, HY2), sh2[0], sh2[1])
                mg.see("cn", np.abs(cn2 - min_corr))
                cn2[np.isnan(cn2) | (cn2 < min_corr)] = 0
            pnr2 = pnr2.reshape(sh2, order="F")
            res["steps"].append(dict(kind="apply", r=r, c=c, pnr=pnr2.copy(), cn=cn2.copy()))
            PNR[s0:s1, t0:t1] = pnr2; Cn[s0:s1, t0:t1] = cn2
            v_search[s0:s1, t0:t1] = cn2 * pnr2
            v_search[ind_bd] = 0; v_search[ind_search] = 0
            if k == K:
                searching = False
                break
    res["center"] = np.asarray(res["center"], dtype=np.int64).reshape(-1, 2)
    res["Cn"], res["PNR"], res["margins"] = Cn0, PNR0, mg
    return res


# ---- the field of view ----------------------------------------------------------------------------------------------------------------------------------------
def greedy_fov(Y_td, video, gSig, gSiz, nframes=None, bd=3, seeds=None, **kw):
    """initComponents_parallel.m:308-352,410-484 on the geometry of a PatchedVideo: every block on its own with bd = (patch == block) .* bd, the neurons whose
    seed lies in the patch interior kept, patches in column-major order.  seeds: 1-based FOV pixels.  Returns dict(A (d x K), C, C_raw, S, kernel_pars,
    center (K x 2, 1-based FOV), blocks: idx -> the block's result, margins)."""
    d1, d2 = video.d1, video.d2
    n = Y_td.shape[0] if nframes is None else int(nframes)
    cols, C, Craw, S, kp, ctr = [], [], [], [], [], []
    blocks = {}
    mg = Margins()
    for idx in video.order:
        pp, bp = [int(x) for x in video.patch_pos[idx]], [int(x) for x in video.block_pos[idx]]
        nr, nc = bp[1] - bp[0] + 1, bp[3] - bp[2] + 1
        Yb = np.asarray(Y_td[:n][:, video.block_pix[idx]], dtype=np.float64).T
        bd4 = [bd if pp[j] == bp[j] else 0 for j in range(4)]
        loc = None
        if seeds is not None:
            loc = [(r - bp[0], c - bp[2]) for (r, c) in seeds if bp[0] <= r <= bp[1] and bp[2] <= c <= bp[3]]
        res = blocks[idx] = greedy_block(Yb, nr, nc, gSig, gSiz, bd4=bd4, seeds=loc, **kw)
        for key, val in res["margins"].items():
            mg.see(key, val)
        for k in range(res["center"].shape[0]):
            r, c = res["center"][k, 0] + bp[0] - 1, res["center"][k, 1] + bp[2] - 1
            if not (pp[0] <= r <= pp[1] and pp[2] <= c <= pp[3]):
                continue
            (r0, r1, c0, c1), ai = res["A"][k]
            img = np.zeros((d1, d2))
            img[r0 + bp[0] - 1:r1 + bp[0] - 1, c0 + bp[2] - 1:c1 + bp[2] - 1] = ai
            cols.append(img.reshape(-1, order="F")); C.append(res["C"][k]); Craw.append(res["C_raw"][k]); S.append(res["S"][k]); kp.append(res["kernel_pars"][k])
            ctr.append((r, c))
    K = len(cols)
    return dict(A=np.stack(cols, axis=1) if K else np.zeros((d1 * d2, 0)), C=np.array(C).reshape(K, n), C_raw=np.array(Craw).reshape(K, n), S=S, kernel_pars=kp,
                center=np.asarray(ctr, dtype=np.int64).reshape(-1, 2), blocks=blocks, margins=mg)
