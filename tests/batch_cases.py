"""TEST INFRASTRUCTURE: the fixtures and float64 restatements of the batch-mode tests (tests/test_batch_host.py on the CPU, tests/test_gpu_batch.py on the engine).

One synthetic recording of a 32 x 32 field of view (cnmf_e_amd/synth.py: footprints, background field and noise) is cut into three temporal batches of 96, 128 and
80 frames -- unequal, no multiple of each other, all >= 64.  The traces are this file's own, so that every neuron fires in every batch: per neuron and batch eight
spikes at seeded frames, AR(1) decay 0.9.  Case "late" has a sixth neuron that is silent throughout batch 1 and fires in batches 2 and 3.

Of these 32 x 32 cases no test relies on WHICH neurons the greedy passes pick (the small field of view's background blobs are neuron-sized, and a lone neuron of
this size gives fewer than the ten seed pixels greedyROI_endoscope's K = numel(seeds) / 10 needs to start a search in a residual): the GPU tests compare two ways of
running the same calls, and restate what the batch methods add.

K GROWING ACROSS BATCHES by the search itself has a fixture of its own, GROW: the same three batch lengths on a 40 x 36 field of view with ring radius 8 and neurons of
gSig = 2, gSiz = 9 (a ring of radius 6 passes through the footprints of the pixels next to the centre and sharpens the footprint the search extracts: the float64
oracle's then correlates 0.6-0.8 with the truth, at radius 8 above 0.96), four neurons of which the last is silent throughout batch 1 and fires in batches 2 and 3; min_corr = 0.5,
min_pnr = 4 and four spikes of amplitude 20-30 (AR(1) decay 0.95) per neuron and batch, chosen so that the late neuron's seed passes with margin AND brings more than the
ten seed pixels the search needs.  The condition on the fixture is checked on the CPU (tests/test_batch_host.py::test_grow_fixture, grow_oracle_check below) with
tests/greedy_oracle.py: greedy_fov on batch 1's video accepts no centre within 3 pixels of the late neuron's; greedy_block on batch 2's residual -- the float64 oracle's
after one background update against the three other neurons (their synth start A_init, C_init: OracleSources2D.init_residual) -- accepts one there, with Cn * PNR at that
seed at least 1.5 x min_corr * min_pnr, and the footprint it extracts correlates above 0.9 with the truth.  GROW_RECORDED holds what that check gave."""
import dataclasses
import os
import sys

import numpy as np
import scipy.sparse as sp

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for p in (HERE, os.path.join(ROOT, "oracle")):
    if p not in sys.path:
        sys.path.insert(0, p)

from cnmf_e_amd import synth

D1 = D2 = 32
RADIUS = 4
GSIG, GSIZ = 1.5, 7
BD = 3
MIN_CORR, MIN_PNR = 0.6, 6.0
NSPK, AMP = 8, (20.0, 30.0)               # spikes per neuron and batch, their amplitudes
CUTS = (96, 128, 80)                      # frames per batch
T = sum(CUTS)
CASES = {
    "plain": dict(K=5, seed=11, late=None),
    "late": dict(K=6, seed=11, late=5),   # neuron 5 (0-based) is silent in batch 1
}

_made = {}


def ranges():
    """the batches' frame ranges, 0-based half-open"""
    e = np.concatenate([[0], np.cumsum(CUTS)])
    return [(int(e[i]), int(e[i + 1])) for i in range(len(CUTS))]


def make(name):
    """(factors with this file's traces, video (T, d) float32 read-only)"""
    if name not in _made:
        c = CASES[name]
        f = synth.make_factors(D1, D2, T, c["K"], c["seed"], gSig=GSIG, gSiz=GSIZ, min_sep=6)
        rng = np.random.default_rng(1000 + c["seed"])
        drive = np.zeros((c["K"], T))
        for k in range(c["K"]):
            for b, (t0, t1) in enumerate(ranges()):
                if c["late"] == k and b == 0:
                    continue
                frames = t0 + 4 + rng.choice(t1 - t0 - 24, size=NSPK, replace=False)      # (room for the decay inside the batch)
                drive[k, frames] = rng.uniform(AMP[0], AMP[1], NSPK)
        C = synth._ar1(drive, 0.9)
        if c["late"] is not None:
            C[c["late"], :CUTS[0]] = 0.0
        f = dataclasses.replace(f, C_true=C.astype(np.float32), C_init=np.maximum(C + rng.normal(0.0, 0.5, C.shape), 0.0).astype(np.float32))
        Y = synth.make_video(f, np.float32)
        Y.setflags(write=False)
        _made[name] = (f, Y)
    return _made[name]


def options(deconv=False, **extra):
    from cnmf_e_amd.sources2d import Options
    return Options(d1=D1, d2=D2, ring_radius=RADIUS, gSig=GSIG, gSiz=GSIZ, bd=BD, min_corr=MIN_CORR, min_pnr=MIN_PNR, maxIter=3, deconv_flag=bool(deconv), **extra)


class _Geometry:
    def create_patch(self, *a):
        pass


def geometry(n_frames, pdims):
    from cnmf_e_amd.sources2d import PatchedVideo
    return PatchedVideo(D1, D2, n_frames, pdims, RADIUS, _Geometry())


def centre_of(f, k):
    """the brightest pixel of true footprint k, 1-based (row, column)"""
    p = int(np.argmax(np.asarray(f.A_true[:, [k]].todense()).ravel()))
    return p % D1 + 1, p // D1 + 1


# ---- float64 restatements ------------------------------------------------------------------------------------------------------------------------------------
def frame_ranges_by_hand():
    """batch_frame_ranges cases worked by hand from Sources2D.m:298-318: (T, batch_frames) -> ranges"""
    return {
        (1000, 300): [(1, 333), (334, 666), (667, 1000)],      # round(3.33) = 3; round(linspace(1, 1000, 4)) = [1 334 667 1000]
        (100, 40): [(1, 33), (34, 66), (67, 100)],              # round(2.5) = 3 in MATLAB (Python: 2); round(linspace(1, 100, 4)) = [1 34 67 100]
        (50, 80): [(1, 50)],                                    # round(0.625) = 1: one batch
        (77, None): [(1, 77)],
    }


def weighted_average(A_list, C_list):
    """update_spatial_batch.m:18-33 in float64: (A d x K dense float64 with an all-zero column where no batch has energy, the indices of those columns)"""
    cc = np.array([(np.asarray(C, dtype=np.float64) ** 2).sum(axis=1) for C in C_list])
    acc = np.zeros(A_list[0].shape, dtype=np.float64)
    for A, w in zip(A_list, cc):
        Ad = np.asarray(sp.csc_matrix(A).astype(np.float64).todense())
        Ad[:, w == 0] = 0.0
        acc += Ad * w[None, :]
    tot = cc.sum(axis=0)
    dead = np.flatnonzero(~(tot > 0))
    with np.errstate(divide="ignore", invalid="ignore"):
        out = acc / tot[None, :]
    out[:, dead] = 0.0
    return out, dead


def within_one_ulp(got32, want64):
    """every entry of the float32 array lies within one float32 ulp of the float64 value rounded to float32"""
    w = np.asarray(want64, dtype=np.float64).astype(np.float32)
    g = np.asarray(got32, dtype=np.float32)
    return bool(np.all((g == w) | (g == np.nextafter(w, np.float32(np.inf))) | (g == np.nextafter(w, np.float32(-np.inf)))))


# ---- K grows across batches ----------------------------------------------------------------------------------------------------------------------------------
GROW = dict(dims=(40, 36), r=8, gSig=2.0, gSiz=9, K=4, late=3, seed=5, nspk=4, amp=(20.0, 30.0), decay=0.95, min_corr=0.5, min_pnr=4.0, min_sep=8)
# grow_oracle_check() on the CPU (float64): the late neuron's centre (1-based), the distance of the nearest centre batch 1's greedy search accepted, the centre batch 2's
# residual search accepted for it, Cn * PNR at that seed, the threshold min_corr * min_pnr, the seed pixels (Cn >= min_corr and PNR >= min_pnr) of that residual, and the correlation of the extracted footprint with the truth
GROW_RECORDED = dict(centre=(7, 31), nearest_batch1=15.0, found=(8, 31), cn_pnr=6.04, threshold=2.0, seed_pixels=25, footprint_corr=0.964)


def make_grow():
    """(factors, video (T, d) float32 read-only) of GROW"""
    if "grow" not in _made:
        c = GROW
        f = synth.make_factors(c["dims"][0], c["dims"][1], T, c["K"], c["seed"], gSig=c["gSig"], gSiz=c["gSiz"], min_sep=c["min_sep"])
        rng = np.random.default_rng(1000 + c["seed"])
        drive = np.zeros((c["K"], T))
        for k in range(c["K"]):
            for b, (t0, t1) in enumerate(ranges()):
                if c["late"] == k and b == 0:
                    continue
                frames = t0 + 4 + rng.choice(t1 - t0 - 24, size=c["nspk"], replace=False)
                drive[k, frames] = rng.uniform(c["amp"][0], c["amp"][1], c["nspk"])
        C = synth._ar1(drive, c["decay"])
        C[c["late"], :CUTS[0]] = 0.0
        f = dataclasses.replace(f, C_true=C.astype(np.float32), C_init=np.maximum(C + rng.normal(0.0, 0.5, C.shape), 0.0).astype(np.float32))
        Y = synth.make_video(f, np.float32)
        Y.setflags(write=False)
        _made["grow"] = (f, Y)
    return _made["grow"]


def grow_options(deconv=True):
    from cnmf_e_amd.sources2d import Options
    c = GROW
    return Options(d1=c["dims"][0], d2=c["dims"][1], ring_radius=c["r"], gSig=c["gSig"], gSiz=c["gSiz"], bd=BD, min_corr=c["min_corr"], min_pnr=c["min_pnr"], maxIter=3,
                   deconv_flag=bool(deconv))


def grow_centre():
    f, _ = make_grow()
    p = int(np.argmax(np.asarray(f.A_true[:, [GROW["late"]]].todense()).ravel()))
    return p % GROW["dims"][0] + 1, p // GROW["dims"][0] + 1


def grow_oracle_check():
    """the CPU side of the fixture's condition -> dict(centre, nearest_batch1, found (None: not found), cn_pnr, threshold, seed_pixels, footprint_corr)"""
    import cnmfe_oracle as orc
    import greedy_oracle as go
    import residual_cases as rc
    from cnmf_e_amd.sources2d import PatchedVideo
    c = GROW
    d1, d2 = c["dims"]
    f, Y = make_grow()
    ctr = grow_centre()
    t0, t1 = ranges()[0]
    g1 = go.greedy_fov(Y[t0:t1], PatchedVideo(d1, d2, t1 - t0, [d1, d2], c["r"], _Geometry()), c["gSig"], c["gSiz"], bd=BD, min_corr=c["min_corr"], min_pnr=c["min_pnr"])
    nearest = min([float(np.hypot(q[0] - ctr[0], q[1] - ctr[1])) for q in g1["center"]] + [np.inf])
    t0, t1 = ranges()[1]
    known = [k for k in range(c["K"]) if k != c["late"]]
    o = orc.OracleSources2D(Y[t0:t1].T.reshape(d1, d2, t1 - t0, order="F"), d1, d2, t1 - t0, [d1, d2], c["r"], f.A_init.tocsc()[:, known].astype(np.float32),
                            f.C_init[known][:, t0:t1], f.sn, maxIter=3)
    o.update_background_parallel()
    res = rc.collect(dict(dims=c["dims"], gSig=c["gSig"], gSiz=c["gSiz"], min_corr=c["min_corr"], min_pnr=c["min_pnr"], T=t1 - t0), o, o.init_residual)
    blk = res["blocks"][(0, 0)]
    hit = [tuple(int(x) for x in q) for q in res["center"] if np.hypot(q[0] - ctr[0], q[1] - ctr[1]) <= 3]
    v = blk["Cn"] * blk["PNR"]
    truth = np.asarray(f.A_true[:, [c["late"]]].todense()).ravel()
    j = [i for i, q in enumerate(res["center"]) if np.hypot(q[0] - ctr[0], q[1] - ctr[1]) <= 3]
    fc = float(np.corrcoef(res["A"][:, j[0]], truth)[0, 1]) if j else float("nan")
    return dict(footprint_corr=fc, centre=ctr, nearest_batch1=nearest, found=hit[0] if hit else None, cn_pnr=float(v[hit[0][0] - 1, hit[0][1] - 1]) if hit else float("nan"),
                threshold=c["min_corr"] * c["min_pnr"], seed_pixels=int(((blk["Cn"] >= c["min_corr"]) & (blk["PNR"] >= c["min_pnr"])).sum()))
