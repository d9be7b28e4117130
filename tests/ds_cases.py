"""TEST INFRASTRUCTURE: the fixtures of the down-sampled initialisation (options.ssub / options.tsub): tests/test_ds_oracle.py checks their decision margins on
the CPU, tests/test_gpu_ds.py runs them on the engine.  Seeded fp32 videos from synth.make_factors / make_video, the float64 oracle's runs (tests/ds_oracle.py)
cached per case.

The synthetic seed of every case was found by scanning seeds on the CPU until the oracle's decision margins cleared greedy_cases.MARGIN_MIN / MARGIN_DEFAULT for
the automatic search AND for the forced-seed run of the accepted centres, at least two neurons were accepted, and at most 10 % of the field of view was left
out of the Cn comparison of the seed images (ds_oracle.seed_images_fov).  All cases are synthesised at the synthesiser's default noise of 1 (none needed the
raised noise_sd of greedy_cases' case E; case U holds two true neurons instead of three: with three, 400 seeds held none whose updated boxes -- 300 frames
at full resolution -- stayed 1e-4 Sn clear of the 3 Sn threshold).  The cases are the smallest that reach every branch:
    P   four blocks with halo, block sizes ssub does and does not divide, Ts = 201 (Ts % 4 = 1), one frame dropped
    Q   per-dimension scales that are not 1 / 3 (45 -> 15 rows is, 37 -> 13 columns is not), mirrored border taps, center * ssub - 1
    R   tsub = 3: the bins straddle the input quads
    S   nk = 3: the pre-detrend; 600 frames are no multiple of 16
    U   deconv_flag with the DECONV options: S comes back bicubically"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import ds_oracle as dso
from greedy_cases import DECONV, MARGIN_DEFAULT, MARGIN_MIN        # noqa: F401  (the fixture bounds are the ones of the full-resolution fixtures)
from cnmf_e_amd import synth

CASES = {
    "P": dict(dims=(44, 40), T=403, K=3, seed=311, gSig=3.0, gSiz=13, pdims=[22, 20], r=5, ssub=2, tsub=2),
    "Q": dict(dims=(45, 37), T=403, K=3, seed=30, gSig=3.0, gSiz=13, pdims=None, r=5, ssub=3, tsub=1),
    "R": dict(dims=(40, 36), T=600, K=3, seed=250, gSig=2.0, gSiz=9, pdims=None, r=8, ssub=1, tsub=3),
    "S": dict(dims=(40, 36), T=600, K=3, seed=1, gSig=3.0, gSiz=13, pdims=None, r=8, ssub=2, tsub=4, nk=3),
    "U": dict(dims=(40, 36), T=600, K=2, seed=38, gSig=2.0, gSiz=9, pdims=None, r=8, ssub=1, tsub=2, deconv=True),
}
_inputs, _oracle, _images = {}, {}, {}


class _Geometry:
    def create_patch(self, *a):
        pass


def geometry(name):
    from cnmf_e_amd.sources2d import PatchedVideo
    c = CASES[name]
    d1, d2 = c["dims"]
    return PatchedVideo(d1, d2, c["T"], c["pdims"] or [d1, d2], c["r"], _Geometry())


def inputs(name, seed=None):
    key = (name, seed)
    if key not in _inputs:
        c = CASES[name]
        f = synth.make_factors(c["dims"][0], c["dims"][1], c["T"], c["K"], c["seed"] if seed is None else seed, gSig=c["gSig"], gSiz=c["gSiz"],
                               noise_sd=c.get("noise_sd", 1.0))
        Y = synth.make_video(f, np.float32)
        Y.setflags(write=False)
        _inputs[key] = (f, Y)
    return _inputs[key]


def oracle(name, forced=False, seed=None):
    """the oracle's run of a case: the automatic search, or (forced) the forced-seed run of the automatic search's accepted centres.  Computed once, shared."""
    key = (name, forced, seed)
    if key not in _oracle:
        c = CASES[name]
        _, Y = inputs(name, seed)
        kw = dict(nk=c.get("nk", 1), deconv_opts=DECONV if c.get("deconv") else None)
        seeds = [tuple(int(x) for x in rc) for rc in oracle(name, seed=seed)["center"]] if forced else None
        _oracle[key] = dso.greedy_fov_ds(Y, geometry(name), c["gSig"], c["gSiz"], c["ssub"], c["tsub"], seeds=seeds, **kw)
    return _oracle[key]


def oracle_images(name, seed=None):
    """(Cn, PNR, robust) of correlation_pnr_parallel, d1 x d2 each"""
    key = (name, seed)
    if key not in _images:
        c = CASES[name]
        _, Y = inputs(name, seed)
        res = dso.seed_images_fov(Y, geometry(name), c["gSig"], c["gSiz"], c["ssub"], c["tsub"], True, c.get("nk", 1), 3.0)
        for a in res:
            a.setflags(write=False)
        _images[key] = res
    return _images[key]


def margins_clear(mg):
    return all(v >= MARGIN_MIN.get(k, MARGIN_DEFAULT) for k, v in mg.items())


def options(name, **extra):
    from cnmf_e_amd.sources2d import Options
    c = CASES[name]
    return Options(ring_radius=c["r"], gSig=c["gSig"], gSiz=c["gSiz"], nk=c.get("nk", 1), deconv_flag=bool(c.get("deconv")), maxIter=3, ssub=c["ssub"],
                   tsub=c["tsub"], **extra)
