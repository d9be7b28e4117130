"""TEST INFRASTRUCTURE: float64 NumPy restatement of the down-sampled seed images and first initialisation (options.ssub / options.tsub),
    utilities/dsData.m:29-43, endoscope/greedyROI_endoscope.m:46-61,464-487, @Sources2D/correlation_pnr_parallel.m:81-100,
    @Sources2D/initComponents_parallel.m:341-343 (the block is detrended BEFORE greedyROI_endoscope down-samples it)
from the RAW video as the reference sees it.  imresize is restated from the toolbox's documented `contributions` rule, one output sample at a time (output
sample x sits at u = x / scale + (1 - 1 / scale) / 2, scale = out / in per dimension; shrinking stretches the kernel by 1 / scale; taps are mirrored at the
border, [1:n n:-1:1]; every row of weights is normalised).  Built on tests/seed_oracle.py and tests/greedy_oracle.py; nothing here is imported by the product."""
import math
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)

import greedy_oracle as go
import seed_oracle as so


def _box(x):
    return 1.0 if -0.5 <= x < 0.5 else 0.0


def _cubic(x):
    ax = abs(x)
    if ax <= 1:
        return 1.5 * ax ** 3 - 2.5 * ax ** 2 + 1
    if ax <= 2:
        return -0.5 * ax ** 3 + 2.5 * ax ** 2 - 4 * ax + 2
    return 0.0


def resize_weights(n_in, n_out, method="bicubic"):
    """the (n_out x n_in) weight matrix of imresize along one dimension, output size given: scale = n_out / n_in"""
    kern, kw = (_box, 1.0) if method == "box" else (_cubic, 4.0)
    scale = n_out / n_in
    stretch = scale < 1
    if stretch:
        kw = kw / scale
    P = int(math.ceil(kw)) + 2
    M = np.zeros((n_out, n_in))
    for o in range(n_out):
        u = (o + 1) / scale + 0.5 * (1 - 1 / scale)
        left = math.floor(u - kw / 2)
        w = np.array([(scale * kern(scale * (u - (left + i)))) if stretch else kern(u - (left + i)) for i in range(P)])
        w = w / w.sum()
        for i in range(P):
            v = (left + i - 1) % (2 * n_in)                                # 0-based virtual index into [1:n n:-1:1]
            M[o, v if v < n_in else 2 * n_in - 1 - v] += w[i]
    return M


def imresize(img, out_size, method="bicubic"):
    """imresize(img, [nr nc], method) on the first two dimensions"""
    img = np.asarray(img, dtype=np.float64)
    out = np.tensordot(resize_weights(img.shape[0], out_size[0], method), img, axes=(1, 0))
    return np.moveaxis(np.tensordot(resize_weights(img.shape[1], out_size[1], method), out, axes=(1, 1)), 0, 1)


def ds_dims(nr, nc, T, ssub, tsub):
    return -(-nr // ssub), -(-nc // ssub), T // tsub


def ds_data(Y3, ssub, tsub):
    """Y_ds = dsData(Y, options) of an nr x nc x T array (dsData.m:29-43)"""
    Y3 = np.asarray(Y3, dtype=np.float64)
    nr, nc, T = Y3.shape
    d1s, d2s, Ts = ds_dims(nr, nc, T, ssub, tsub)
    out = imresize(Y3, (d1s, d2s), "box") if ssub > 1 else Y3
    if tsub > 1:
        out = out[:, :, :Ts * tsub].reshape(d1s, d2s, Ts, tsub).mean(axis=3)
    return out


def ds_block(Yb, nr, nc, ssub, tsub):
    """dsData of a block given as d_b x T (pixels column-major in nr x nc) -> (ds x Ts, d1s, d2s)"""
    Yb = np.asarray(Yb, dtype=np.float64)
    Yds = ds_data(Yb.reshape(nr, nc, Yb.shape[1], order="F"), ssub, tsub)
    return Yds.reshape(-1, Yds.shape[2], order="F"), Yds.shape[0], Yds.shape[1]


def peel_video(Yb, nr, nc, nk, ssub, tsub):
    """the video a down-sampled peel session searches: dsData(detrend(Y)) (initComponents_parallel.m:341-343, then greedyROI_endoscope.m:52)"""
    Y = np.asarray(Yb, dtype=np.float64)
    if nk > 1:
        Y = so.detrend_spline(Y, nk)
    return ds_block(Y, nr, nc, ssub, tsub)


def up_time(X, n, method):
    """imresize(X, [k, n], method) of k x Ts traces (greedyROI_endoscope.m:481-484); the row dimension keeps its size"""
    X = np.asarray(X, dtype=np.float64)
    return X @ resize_weights(X.shape[1], n, method).T


def scaled(gSig, gSiz, ssub, min_pixel=5.0, bd4=(0, 0, 0, 0)):
    """greedyROI_endoscope.m:56-59"""
    return gSig / ssub, so.matlab_round(gSiz / ssub), min_pixel / ssub ** 2, [so.matlab_round(b / ssub) for b in bd4]


# ---- seed images ------------------------------------------------------------------------------------------------------------------------------------------------
def seed_images_ds(Yb, nr, nc, gSig, gSiz, ssub, tsub, center_psf=True, nk=1, sig=3.0):
    """correlation_pnr_parallel.m:81-100 of one block: (Cn, PNR) at full resolution, robust (nr x nc bool): none of the low-resolution pixels a full-resolution
    one is interpolated from is fragile or has a fragile 8-neighbour (seed_oracle.DELTA, decided on the low-resolution grid before the resize)"""
    Yds, d1s, d2s = ds_block(Yb, nr, nc, ssub, tsub)
    cn, pnr, margin = so.seed_images(Yds, d1s, d2s, gSig / ssub, math.ceil(gSiz / ssub), center_psf, nk, sig)
    bad = so.dilate8(margin < so.DELTA)
    if ssub != 1:
        cn, pnr = imresize(cn, (nr, nc)), imresize(pnr, (nr, nc))
        Wr, Wc = np.abs(resize_weights(d1s, nr)) > 0, np.abs(resize_weights(d2s, nc)) > 0
        bad = (Wr.astype(float) @ bad.astype(float) @ Wc.astype(float).T) > 0
    return cn, pnr, ~bad


def seed_images_fov(Y_td, video, gSig, gSiz, ssub, tsub, center_psf=True, nk=1, sig=3.0):
    d = video.d1 * video.d2
    Cn = np.zeros(d); PNR = np.zeros(d); robust = np.zeros(d, dtype=bool)
    for idx in video.order:
        b = video.block_pos[idx]
        nr, nc = int(b[1] - b[0] + 1), int(b[3] - b[2] + 1)
        Yb = np.asarray(Y_td[:, video.block_pix[idx]], dtype=np.float64).T
        cn, pnr, ok = seed_images_ds(Yb, nr, nc, gSig, gSiz, ssub, tsub, center_psf, nk, sig)
        ip = video.ind_patch[idx]
        Cn[video.patch_pix[idx]] = cn.reshape(-1, order="F")[ip]
        PNR[video.patch_pix[idx]] = pnr.reshape(-1, order="F")[ip]
        robust[video.patch_pix[idx]] = ok.reshape(-1, order="F")[ip]
    sh = (video.d1, video.d2)
    return Cn.reshape(sh, order="F"), PNR.reshape(sh, order="F"), robust.reshape(sh, order="F")


# ---- the first initialisation -------------------------------------------------------------------------------------------------------------------------------------
def greedy_block_ds(Yb, nr, nc, gSig, gSiz, ssub, tsub, nk=1, min_pixel=5.0, bd4=(0, 0, 0, 0), seeds=None, **kw):
    """detrend_spline -> dsData -> greedy_oracle.greedy_block(nk = 1, the scaled parameters) -> the up-sampling of greedyROI_endoscope.m:464-487.
    seeds: 0-based pixels of the LOW-RESOLUTION grid.  The result of greedy_block with A as full nr x nc images, center = center * ssub - 1 (ssub != 1), C,
    C_raw, S over all T frames, Cn / PNR resized; `low` keeps the low-resolution run (steps, margins, center)."""
    T = np.asarray(Yb).shape[1]
    Yds, d1s, d2s = peel_video(Yb, nr, nc, nk, ssub, tsub)
    gs, gz, mp, bds = scaled(gSig, gSiz, ssub, min_pixel, bd4)
    low = go.greedy_block(Yds, d1s, d2s, gs, gz, nk=1, min_pixel=mp, bd4=bds, seeds=seeds, **kw)
    k = low["center"].shape[0]
    res = dict(low=low, margins=low["margins"], steps=low["steps"], kernel_pars=low["kernel_pars"], center=low["center"], Cn=low["Cn"], PNR=low["PNR"])
    A = []
    for (r0, r1, c0, c1), ai in low["A"]:
        img = np.zeros((d1s, d2s))
        img[r0:r1, c0:c1] = ai
        A.append(imresize(img, (nr, nc)) if ssub != 1 else img)
    res["A"] = A
    if ssub != 1:
        res["center"] = low["center"] * ssub - 1
        res["Cn"], res["PNR"] = imresize(low["Cn"], (nr, nc)), imresize(low["PNR"], (nr, nc))
    Ts = Yds.shape[1]
    C, Craw = np.array(low["C"]).reshape(k, Ts), np.array(low["C_raw"]).reshape(k, Ts)
    S = np.array(low["S"]).reshape(k, Ts) if k and low["S"][0] is not None else None
    if tsub != 1 and k:
        C, Craw = up_time(C, T, "box"), up_time(Craw, T, "box")
        S = up_time(S, T, "bicubic") if S is not None else None
    elif tsub != 1:
        C, Craw = np.zeros((0, T)), np.zeros((0, T))
    res["C"], res["C_raw"], res["S"] = C, Craw, S
    return res


def greedy_fov_ds(Y_td, video, gSig, gSiz, ssub, tsub, bd=3, seeds=None, **kw):
    """greedy_oracle.greedy_fov with every block initialised by greedy_block_ds.  seeds: 1-based FOV pixels; a block tries the low-resolution pixel
    floor((r - r0) / ssub), floor((c - c0) / ssub) of every seed it holds."""
    d1, d2 = video.d1, video.d2
    n = Y_td.shape[0]
    cols, C, Craw, S, kp, ctr = [], [], [], [], [], []
    blocks = {}
    mg = go.Margins()
    for idx in video.order:
        pp, bp = [int(x) for x in video.patch_pos[idx]], [int(x) for x in video.block_pos[idx]]
        nr, nc = bp[1] - bp[0] + 1, bp[3] - bp[2] + 1
        Yb = np.asarray(Y_td[:, video.block_pix[idx]], dtype=np.float64).T
        bd4 = [bd if pp[j] == bp[j] else 0 for j in range(4)]
        loc = None
        if seeds is not None:
            loc = [((r - bp[0]) // ssub, (c - bp[2]) // ssub) for (r, c) in seeds if bp[0] <= r <= bp[1] and bp[2] <= c <= bp[3]]
        res = blocks[idx] = greedy_block_ds(Yb, nr, nc, gSig, gSiz, ssub, tsub, bd4=bd4, seeds=loc, **kw)
        for key, val in res["margins"].items():
            mg.see(key, val)
        for k in range(res["center"].shape[0]):
            r, c = res["center"][k, 0] + bp[0] - 1, res["center"][k, 1] + bp[2] - 1
            if not (pp[0] <= r <= pp[1] and pp[2] <= c <= pp[3]):
                continue
            img = np.zeros((d1, d2))
            img[bp[0] - 1:bp[1], bp[2] - 1:bp[3]] = res["A"][k]
            cols.append(img.reshape(-1, order="F")); C.append(res["C"][k]); Craw.append(res["C_raw"][k]); kp.append(res["kernel_pars"][k])
            S.append(res["S"][k] if res["S"] is not None else None)
            ctr.append((r, c))
    K = len(cols)
    return dict(A=np.stack(cols, axis=1) if K else np.zeros((d1 * d2, 0)), C=np.array(C).reshape(K, n), C_raw=np.array(Craw).reshape(K, n), S=S, kernel_pars=kp,
                center=np.asarray(ctr, dtype=np.int64).reshape(-1, 2), blocks=blocks, margins=mg)
