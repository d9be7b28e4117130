"""TEST INFRASTRUCTURE: float64 NumPy restatement of the seed images [Cn, PNR] of one block,
    @Sources2D/correlation_pnr_parallel.m:70-128 -> endoscope/correlation_image_endoscope.m:36-96 -> utilities/correlation_image.m:31-77
    (+ endoscope/detrend_data.m:22-29 for nk > 1), from the RAW video as the reference sees it.
Independent of the product: its own fspecial / imfilter restatements (an even kernel is filtered about imfilter's origin floor((n + 1) / 2), not padded),
scipy's B-spline design matrix for the detrend basis, oasis_oracle.GetSn for the noise.  Nothing here is imported by the product."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
for p_ in (os.path.join(os.path.dirname(HERE), "oracle"),):
    if p_ not in sys.path:
        sys.path.insert(0, p_)

import oasis_oracle as oo

DELTA = 1e-4          # a pixel whose margin min_t |HY(t) - sig Sn| / Sn is below this is FRAGILE: its threshold decisions may differ under fp32 rounding


def fspecial_gaussian(n, sigma):
    x = np.arange(n, dtype=np.float64) - (n - 1) / 2.0
    h = np.exp(-(x[:, None] ** 2 + x[None, :] ** 2) / (2.0 * sigma ** 2))
    h[h < np.finfo(np.float64).eps * h.max()] = 0.0
    return h / h.sum()


def matlab_round(x):
    return int(np.sign(x) * np.floor(abs(x) + 0.5))


def make_psf(gSig, gSiz, center_psf):
    """correlation_image_endoscope.m:36-47 (the raw kernel: even sizes stay even)"""
    if gSig <= 0:
        return None
    if center_psf:
        psf = fspecial_gaussian(int(np.ceil(gSig * 4 + 1)), gSig)
        ind = psf >= psf[:, 0].max()
        psf = psf - psf[ind].mean()
        psf[~ind] = 0.0
        return psf
    return fspecial_gaussian(matlab_round(gSiz), gSig)


def imfilter_replicate(Y3, psf):
    """imfilter(Y, psf, 'replicate'): correlation, HY(r, c) = sum_ij psf(i, j) Y(r + i - cr, c + j - cc) with the origin (cr, cc) = floor((n + 1) / 2) (1-based)"""
    n0, n1 = psf.shape
    cr, cc = (n0 + 1) // 2 - 1, (n1 + 1) // 2 - 1
    nr, nc = Y3.shape[:2]
    Yp = np.pad(Y3, ((cr, n0 - 1 - cr), (cc, n1 - 1 - cc), (0, 0)), mode="edge")
    out = np.zeros_like(Y3)
    for i in range(n0):
        for j in range(n1):
            if psf[i, j] != 0:
                out += psf[i, j] * Yp[i:i + nr, j:j + nc]
    return out


def detrend_spline(Y, nk):
    """detrend_data.m:22-29: X = bsplineM((1:T)', linspace(1, T, nk), 4); R = (Y X) / (X' X); Ydt = Y - R X'"""
    from scipy.interpolate import BSpline
    T = Y.shape[1]
    br = np.linspace(1.0, float(T), nk)
    X = BSpline.design_matrix(np.arange(1, T + 1, dtype=np.float64), np.r_[[br[0]] * 3, br, [br[-1]] * 3], 3).toarray()
    R = np.linalg.solve(X.T @ X, X.T @ Y.T).T
    return Y - R @ X.T


def filtered_traces(Yb, nr, nc, gSig, gSiz, center_psf=True, nk=1, sig=3.0):
    """(HY thresholded (d_b x T), PNR (d_b), margin (d_b)) of a block Yb (d_b x T, pixels column-major in an nr x nc image)"""
    Y = np.asarray(Yb, dtype=np.float64)
    T = Y.shape[1]
    if nk > 1:
        Y = detrend_spline(Y, nk)                                          # correlation_pnr_parallel.m:91-93
    psf = make_psf(gSig, gSiz, center_psf)
    Y3 = Y.reshape(nr, nc, T, order="F")
    HY = (imfilter_replicate(Y3, psf) if psf is not None else Y3).reshape(nr * nc, T, order="F")   # :78-84
    HY = HY - np.median(HY, axis=1, keepdims=True)                         # :85
    mx = HY.max(axis=1)                                                    # :86
    Sn = np.array([oo.GetSn(row) for row in HY])                           # :87
    margin = np.abs(HY - sig * Sn[:, None]).min(axis=1) / Sn
    HY = np.where(HY < sig * Sn[:, None], 0.0, HY)                         # :93
    return HY, mx / Sn, margin


def correlation_image(HY, nr, nc):
    """correlation_image(HY, [1, 2], nr, nc): utilities/correlation_image.m:31-77 -- sz = [1, 2] is the 8 neighbours; zero padding, divided by the count"""
    Z = HY - HY.mean(axis=1, keepdims=True)
    sY = np.sqrt((Z * Z).mean(axis=1))
    sY[sY == 0] = 1.0
    Z = (Z / sY[:, None]).reshape(nr, nc, -1, order="F")
    Zp = np.pad(Z, ((1, 1), (1, 1), (0, 0)))
    Mp = np.pad(np.ones((nr, nc)), 1)
    S = np.zeros_like(Z); cnt = np.zeros((nr, nc))
    for dr in (-1, 0, 1):
        for dc in (-1, 0, 1):
            if dr or dc:
                S += Zp[1 + dr:1 + dr + nr, 1 + dc:1 + dc + nc]
                cnt += Mp[1 + dr:1 + dr + nr, 1 + dc:1 + dc + nc]
    return (S * Z).mean(axis=2) / cnt


def dilate8(mask):
    """the pixels that are set or have a set pixel among their 8 neighbours"""
    nr, nc = mask.shape
    mp = np.pad(mask, 1)
    out = np.zeros_like(mask)
    for dr in (-1, 0, 1):
        for dc in (-1, 0, 1):
            out |= mp[1 + dr:1 + dr + nr, 1 + dc:1 + dc + nc]
    return out


def seed_images(Yb, nr, nc, gSig, gSiz, center_psf=True, nk=1, sig=3.0):
    """(Cn, PNR, margin) as nr x nc images of one block"""
    HY, pnr, margin = filtered_traces(Yb, nr, nc, gSig, gSiz, center_psf, nk, sig)
    Cn = correlation_image(HY, nr, nc)
    return Cn, pnr.reshape(nr, nc, order="F"), margin.reshape(nr, nc, order="F")


def seed_images_fov(Y_td, video, gSig, gSiz, center_psf=True, nk=1, sig=3.0, nframes=None):
    """correlation_pnr_parallel.m:70-128 on the geometry of a PatchedVideo: every block on its own, the patch interiors scattered into the d1 x d2 images.
    Returns (Cn, PNR, robust): robust = pixels none of whose block-local 3 x 3 neighbourhood is fragile (decided inside the block that owns the pixel)."""
    d = video.d1 * video.d2
    Cn = np.zeros(d); PNR = np.zeros(d); robust = np.zeros(d, dtype=bool)
    n = Y_td.shape[0] if nframes is None else int(nframes)
    for idx in video.order:
        b = video.block_pos[idx]
        nr, nc = int(b[1] - b[0] + 1), int(b[3] - b[2] + 1)
        Yb = np.asarray(Y_td[:n][:, video.block_pix[idx]], dtype=np.float64).T
        cn, pnr, margin = seed_images(Yb, nr, nc, gSig, gSiz, center_psf, nk, sig)
        ok = ~dilate8(margin < DELTA)
        ip = video.ind_patch[idx]
        Cn[video.patch_pix[idx]] = cn.reshape(-1, order="F")[ip]
        PNR[video.patch_pix[idx]] = pnr.reshape(-1, order="F")[ip]
        robust[video.patch_pix[idx]] = ok.reshape(-1, order="F")[ip]
    sh = (video.d1, video.d2)
    return Cn.reshape(sh, order="F"), PNR.reshape(sh, order="F"), robust.reshape(sh, order="F")
