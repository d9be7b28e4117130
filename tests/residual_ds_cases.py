"""TEST INFRASTRUCTURE: the fixtures of the DOWN-SAMPLED second pass (options.ssub / options.tsub in Sources2D.initComponents_residual_parallel;
tests/test_residual_ds_oracle.py checks their decision margins on the CPU, tests/test_gpu_init_residual_ds.py runs them on the engine), in the style of
tests/residual_cases.py: seeded fp32 videos whose model WITHHOLDS the last `hold` neurons, one background update, BD = 3, MIN_SEP = 5, and the float64 oracle's
second pass per patch as the composition
    oracle/cnmfe_oracle.py::OracleSources2D.init_residual(idx)  ->  tests/ds_oracle.py::greedy_block_ds(R, nr_patch, nc_patch, ..., ssub, tsub, nk=1, bd4=..., K=...)
(@Sources2D/initComponents_residual_parallel.m:171-177,232 hands greedyROI_endoscope the patch residual and the options; greedyROI_endoscope.m:46-61,464-487
down-samples it, scales gSig, gSiz, min_pixel, bd and brings the results back up).

The synthetic seed of every case was found with scripts/residual_ds_seed_scan.py: seeds scanned on the CPU until the automatic run and the forced-seed run accept
the same >= 2 centres and every decision margin clears TWICE the bounds of tests/greedy_cases.py.  At min_corr = 0.6 (tests/residual_cases.py) no seed of 48 finds
a neuron at ssub = 2 -- the reference caps K at floor(#(v_search > 0) / 10) and a quarter of the pixels survive --, hence min_corr = 0.3 with gSig = 3, gSiz = 13.
With bg_ssub = 2 the coarser background leaves more in the residual and the search makes many more, tighter decisions: none of 40 to 60 seeds was a candidate at
48 x 44 (2, 2), 45 x 37 (2, 1) or 40 x 36 (1, 2).  Case G therefore calls the method with K = Kmax = 2 new neurons per patch (the method's own argument), which ends
the search after the second neuron; seed 60 of 64 is then a candidate."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import ds_oracle as dso
import greedy_cases as gc
import greedy_oracle as go
import residual_cases as rc

#   K = true neurons of the synthetic video, the last `hold` of them unknown to the model
CASES = {
    "A": dict(dims=(48, 44), T=402, K=5, hold=3, seed=0, gSig=3.0, gSiz=13, pdims=None, r=8, min_corr=0.3, min_pnr=5.0, ssub=2, tsub=2),       # Ts = 201, Ts % 4 = 1
    "B": dict(dims=(64, 60), T=402, K=8, hold=4, seed=33, gSig=3.0, gSiz=13, pdims=[32, 30], r=8, min_corr=0.3, min_pnr=5.0, ssub=2, tsub=3),   # 2 x 2 patches: bd differs per patch, Ts = 134
    "C": dict(dims=(45, 37), T=403, K=5, hold=3, seed=7, gSig=3.0, gSiz=13, pdims=None, r=8, min_corr=0.3, min_pnr=5.0, ssub=2, tsub=1),       # ssub does not divide: mirrored taps
    "D": dict(dims=(57, 49), T=400, K=5, hold=3, seed=2, gSig=4.0, gSiz=17, pdims=None, r=10, min_corr=0.3, min_pnr=5.0, ssub=3, tsub=2),      # per-dimension scales, center * 3 - 1
    "E": dict(dims=(40, 36), T=600, K=4, hold=2, seed=7, gSig=2.0, gSiz=9, pdims=None, r=6, min_corr=0.6, min_pnr=5.0, ssub=1, tsub=3),        # bins straddle the input quads
    "F": dict(dims=(48, 44), T=402, K=5, hold=3, seed=8, gSig=3.0, gSiz=13, pdims=None, r=8, min_corr=0.3, min_pnr=5.0, ssub=2, tsub=2, deconv=True),
    "G": dict(dims=(45, 37), T=403, K=5, hold=3, seed=60, gSig=3.0, gSiz=13, pdims=None, r=8, min_corr=0.3, min_pnr=5.0, ssub=2, tsub=1, bg_ssub=2, Kmax=2),      # the imresize form of the background; at most Kmax new neurons per patch
}
MIN_SEP = rc.MIN_SEP
BD = rc.BD
MARGIN_FACTOR = 2.0     # a candidate seed clears twice the bounds of tests/greedy_cases.py on the oracle's own residual
_inputs, _fit, _oracle = {}, {}, {}


def pdims(c):
    return rc.pdims(c)


def inputs(name, case=None):
    """(factors, video (T, d) fp32 read-only, A0 (d x K - hold), C0) -- residual_cases.inputs, kept per case name"""
    if case is not None:
        return rc.inputs(name, case)
    if name not in _inputs:
        _inputs[name] = rc.inputs(name, CASES[name])
    return _inputs[name]


def oracle_object(name, case=None):
    """a FRESH OracleSources2D of the case after one update_background_parallel (the W, b0 of that fit are computed once per case name and copied in)"""
    if case is not None:
        return rc.oracle_object(name, case)
    c = CASES[name]
    if name not in _fit:
        o = rc.oracle_object(name, c)
        _fit[name] = ({k: v.copy() for k, v in o.W.items()}, {k: v.copy() for k, v in o.b0.items()})
        return o
    import cnmfe_oracle as orc
    f, Y, A0, C0 = inputs(name)
    d1, d2 = c["dims"]
    o = orc.OracleSources2D(Y.T.reshape(d1, d2, c["T"], order="F"), d1, d2, c["T"], pdims(c), c["r"], A0.astype(np.float32), C0, f.sn, maxIter=3,
                            bg_ssub=c.get("bg_ssub", 1))
    W, b0 = _fit[name]
    o.W = {k: v.copy() for k, v in W.items()}; o.b0 = {k: v.copy() for k, v in b0.items()}
    o.A_prev = o.A.copy(); o.C_prev = o.C.copy()
    return o


def scaled_bd(c, edge):
    """bd of a patch: :173 (options.bd times the edge flags), then greedyROI_endoscope.m:59"""
    return [BD * int(e) for e in edge]


def collect(c, o, source, seeds=None, K=None, low_video=False):
    """the down-sampled second pass over every patch of the oracle object `o` and its collection (:345-398).  source(idx): the patch residual, d_patch x T
    float64 -- or, with low_video, the ALREADY down-sampled video of the patch, d1s d2s x Ts (what the device exported), on which greedy_block runs with the
    scaled parameters and the up-sampling of ds_oracle follows.  seeds: 1-based FOV pixels, tried by the patch that holds them on the low-resolution cell that
    holds them.  Returns dict(blocks, A (d x K_new, FOV), C, C_raw, S, kernel_pars, center (1-based FOV), margins)."""
    d1, d2 = c["dims"]
    ssub, tsub = c["ssub"], c["tsub"]
    cols, C, Craw, S, kp, ctr, blocks = [], [], [], [], [], [], {}
    mg = go.Margins()
    K = c.get("Kmax") if K is None else K
    for idx, pp, edge in rc.patches(o):
        nr, nc = pp[1] - pp[0] + 1, pp[3] - pp[2] + 1
        loc = None if seeds is None else [((r - pp[0]) // ssub, (q - pp[2]) // ssub) for (r, q) in seeds if pp[0] <= r <= pp[1] and pp[2] <= q <= pp[3]]
        kw = dict(min_corr=c["min_corr"], min_pnr=c["min_pnr"], K=nr * nc if K is None else K, deconv_opts=gc.DECONV if c.get("deconv") else None)
        if low_video:
            res = greedy_block_low(np.asarray(source(idx), dtype=np.float64), nr, nc, c["T"], c["gSig"], c["gSiz"], ssub, tsub, bd4=scaled_bd(c, edge), seeds=loc, **kw)
        else:
            res = dso.greedy_block_ds(source(idx), nr, nc, c["gSig"], c["gSiz"], ssub, tsub, nk=1, bd4=scaled_bd(c, edge), seeds=loc, **kw)
        blocks[idx] = res
        for key, val in res["margins"].items():
            mg.see(key, val)
        for k in range(res["center"].shape[0]):
            ai = res["A"][k]
            if not ai.any():
                continue
            img = np.zeros((d1, d2))
            img[pp[0] - 1:pp[1], pp[2] - 1:pp[3]] = ai
            cols.append(img.reshape(-1, order="F")); C.append(res["C"][k]); Craw.append(res["C_raw"][k]); kp.append(res["kernel_pars"][k])
            S.append(res["S"][k] if res["S"] is not None else None)
            ctr.append((res["center"][k, 0] + pp[0] - 1, res["center"][k, 1] + pp[2] - 1))
    Kn = len(cols)
    return dict(A=np.stack(cols, axis=1) if Kn else np.zeros((d1 * d2, 0)), C=np.array(C).reshape(Kn, c["T"]), C_raw=np.array(Craw).reshape(Kn, c["T"]), S=S,
                kernel_pars=kp, center=np.asarray(ctr, dtype=np.int64).reshape(-1, 2), blocks=blocks, margins=mg)


class _Given:
    """ds_oracle.greedy_block_ds on a video that IS the down-sampled one: its dsData step is replaced by the identity for the duration of the call"""
    def __init__(self, Yds, d1s, d2s):
        self.v = (Yds, d1s, d2s)

    def __enter__(self):
        self.keep = dso.peel_video
        dso.peel_video = lambda Yb, nr, nc, nk, ssub, tsub: self.v

    def __exit__(self, *a):
        dso.peel_video = self.keep


def greedy_block_low(Yds, nr, nc, T, gSig, gSiz, ssub, tsub, **kw):
    """greedy_block_ds with the down-sampling already done: Yds is d1s d2s x Ts of the nr x nc patch with T frames"""
    d1s, d2s, Ts = dso.ds_dims(nr, nc, T, ssub, tsub)
    assert Yds.shape == (d1s * d2s, Ts), (Yds.shape, d1s, d2s, Ts)
    with _Given(Yds, d1s, d2s):
        return dso.greedy_block_ds(np.zeros((nr * nc, T)), nr, nc, gSig, gSiz, ssub, tsub, nk=1, **kw)


def oracle(name, forced=False):
    """the oracle's down-sampled second pass of a case on ITS OWN residual: the automatic search, or (forced) the forced-seed run of its accepted centres"""
    key = (name, forced)
    if key not in _oracle:
        o = oracle_object(name)
        seeds = [tuple(int(x) for x in r) for r in oracle(name)["center"]] if forced else None
        _oracle[key] = collect(CASES[name], o, o.init_residual, seeds)
    return _oracle[key]


def margins_clear(mg, factor=1.0):
    return rc.margins_clear(mg, factor)


def options(name, **extra):
    from cnmf_e_amd.sources2d import Options
    c = CASES[name]
    return Options(ring_radius=c["r"], gSig=c["gSig"], gSiz=c["gSiz"], bg_ssub=c.get("bg_ssub", 1), deconv_flag=bool(c.get("deconv")), maxIter=3, bd=BD,
                   ssub=c["ssub"], tsub=c["tsub"], **extra)
