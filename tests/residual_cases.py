"""TEST INFRASTRUCTURE: the fixtures of the residual-initialisation tests (tests/test_residual_oracle.py checks their decision margins on the CPU,
tests/test_gpu_init_residual.py runs them on the engine), in the style of tests/greedy_cases.py: seeded fp32 videos from synth.make_factors / make_video whose model
(A_init, C_init) WITHHOLDS the last `hold` neurons, one background update, and the float64 oracle's second pass per patch,
    oracle/cnmfe_oracle.py::OracleSources2D.init_residual(idx)  ->  tests/greedy_oracle.py::greedy_block(R, nr_patch, nc_patch, ..., nk=1, bd4=..., K=...)
(@Sources2D/initComponents_residual_parallel.m:106-121,165-220; the collection of :345-412 is `collect` below).

The synthetic seed of every case was found with scripts/residual_seed_scan.py: seeds scanned on the CPU until the oracle's decision margins cleared the bounds of
tests/greedy_cases.py (MARGIN_MIN / MARGIN_DEFAULT) for the automatic search AND for the forced-seed run of the accepted centres, with at least two neurons
found.  About 1 seed in 30 does at these shapes; the tight margins are always `pnr` and `hy`."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import greedy_cases as gc
import greedy_oracle as go
import cnmfe_oracle as orc
from cnmf_e_amd import synth

#   K = true neurons of the synthetic video, the last `hold` of them unknown to the model
CASES = {
    "P": dict(dims=(64, 60), T=400, K=8, hold=4, seed=104, gSig=2.0, gSiz=9, pdims=[32, 30], r=6, min_corr=0.6, min_pnr=5.0),                  # 2 x 2 patches: bd differs per patch, T % 4 = 0
    "Q": dict(dims=(40, 36), T=403, K=4, hold=2, seed=0, gSig=2.0, gSiz=9, pdims=None, r=6, min_corr=0.6, min_pnr=5.0),                    # one patch, T % 4 = 3
    "S": dict(dims=(40, 36), T=400, K=4, hold=2, seed=79, gSig=2.0, gSiz=9, pdims=None, r=6, min_corr=0.6, min_pnr=5.0, bg_ssub=2),         # the imresize form of the background
    "D": dict(dims=(40, 36), T=400, K=4, hold=2, seed=99, gSig=2.0, gSiz=9, pdims=None, r=6, min_corr=0.6, min_pnr=5.0, deconv=True),
}
MIN_SEP = 5
BD = 3
_inputs, _oracle_obj, _oracle = {}, {}, {}


def pdims(c):
    return c["pdims"] or list(c["dims"])


def inputs(name, case=None):
    """(factors, video (T, d) fp32 read-only, A0 (d x K - hold), C0): the model withholds the last `hold` neurons"""
    c = case or CASES[name]
    key = name if case is None else None
    if key is None or key not in _inputs:
        f = synth.make_factors(c["dims"][0], c["dims"][1], c["T"], c["K"], c["seed"], gSig=c["gSig"], gSiz=c["gSiz"], min_sep=MIN_SEP)
        Y = synth.make_video(f, np.float32)
        Y.setflags(write=False)
        known = c["K"] - c["hold"]
        out = (f, Y, f.A_init.tocsc()[:, :known], f.C_init[:known])
        if key is None:
            return out
        _inputs[key] = out
    return _inputs[key]


def oracle_object(name, case=None):
    """a FRESH OracleSources2D of the case after one update_background_parallel (the W, b0 of that fit are computed once per case and copied in)"""
    c = case or CASES[name]
    f, Y, A0, C0 = inputs(name, case)
    d1, d2 = c["dims"]
    o = orc.OracleSources2D(Y.T.reshape(d1, d2, c["T"], order="F"), d1, d2, c["T"], pdims(c), c["r"], A0.astype(np.float32), C0, f.sn, maxIter=3,
                            bg_ssub=c.get("bg_ssub", 1))
    if case is not None or name not in _oracle_obj:
        o.update_background_parallel()
        if case is None:
            _oracle_obj[name] = ({k: v.copy() for k, v in o.W.items()}, {k: v.copy() for k, v in o.b0.items()})
    else:
        W, b0 = _oracle_obj[name]
        o.W = {k: v.copy() for k, v in W.items()}; o.b0 = {k: v.copy() for k, v in b0.items()}
        o.A_prev = o.A.copy(); o.C_prev = o.C.copy()
    return o


def patches(o):
    """the patches in MATLAB's linear (column-major) order with their 1-based position and the edge flags of :173"""
    nr, nc = o.patch_pos.shape
    for n in range(nc):
        for m in range(nr):
            yield (m, n), [int(x) for x in o.patch_pos[m, n]], [m == 0, m == nr - 1, n == 0, n == nc - 1]


def collect(c, o, source, seeds=None, K=None):
    """the second pass over every patch of the oracle object `o` on the videos source(idx) (d_patch x T float64) and its collection (:345-398).
    seeds: 1-based FOV pixels, tried by the patch that holds them.  Returns dict(blocks: idx -> greedy_block's result, A (d x K_new, FOV), C, C_raw, S,
    kernel_pars, center (1-based FOV), margins)."""
    d1, d2 = c["dims"]
    cols, C, Craw, S, kp, ctr, blocks = [], [], [], [], [], [], {}
    mg = go.Margins()
    for idx, pp, edge in patches(o):
        nr, nc = pp[1] - pp[0] + 1, pp[3] - pp[2] + 1
        loc = None if seeds is None else [(r - pp[0], q - pp[2]) for (r, q) in seeds if pp[0] <= r <= pp[1] and pp[2] <= q <= pp[3]]
        res = blocks[idx] = go.greedy_block(source(idx), nr, nc, c["gSig"], c["gSiz"], nk=1, min_corr=c["min_corr"], min_pnr=c["min_pnr"],
                                            bd4=[BD * int(e) for e in edge], K=nr * nc if K is None else K,
                                            deconv_opts=gc.DECONV if c.get("deconv") else None, seeds=loc)
        for key, val in res["margins"].items():
            mg.see(key, val)
        for k in range(res["center"].shape[0]):
            (r0, r1, c0, c1), ai = res["A"][k]
            if not ai.any():
                continue
            img = np.zeros((d1, d2))
            img[r0 + pp[0] - 1:r1 + pp[0] - 1, c0 + pp[2] - 1:c1 + pp[2] - 1] = ai
            cols.append(img.reshape(-1, order="F")); C.append(res["C"][k]); Craw.append(res["C_raw"][k]); S.append(res["S"][k]); kp.append(res["kernel_pars"][k])
            ctr.append((res["center"][k, 0] + pp[0] - 1, res["center"][k, 1] + pp[2] - 1))
    Kn = len(cols)
    return dict(A=np.stack(cols, axis=1) if Kn else np.zeros((d1 * d2, 0)), C=np.array(C).reshape(Kn, c["T"]), C_raw=np.array(Craw).reshape(Kn, c["T"]), S=S,
                kernel_pars=kp, center=np.asarray(ctr, dtype=np.int64).reshape(-1, 2), blocks=blocks, margins=mg)


def oracle(name, forced=False):
    """the oracle's second pass of a case on ITS OWN residual: the automatic search, or (forced) the forced-seed run of its accepted centres.  Computed once."""
    key = (name, forced)
    if key not in _oracle:
        o = oracle_object(name)
        seeds = [tuple(int(x) for x in rc) for rc in oracle(name)["center"]] if forced else None
        _oracle[key] = collect(CASES[name], o, o.init_residual, seeds)
    return _oracle[key]


def margins_clear(mg, factor=1.0):
    """the keys of a Margins whose value is below factor x the fixture bound of tests/greedy_cases.py (empty: the fixture pins every decision)"""
    return {k: v for k, v in mg.items() if v < factor * gc.MARGIN_MIN.get(k, gc.MARGIN_DEFAULT)}


def options(name, **extra):
    from cnmf_e_amd.sources2d import Options
    c = CASES[name]
    return Options(ring_radius=c["r"], gSig=c["gSig"], gSiz=c["gSiz"], bg_ssub=c.get("bg_ssub", 1), deconv_flag=bool(c.get("deconv")), maxIter=3, bd=BD, **extra)
