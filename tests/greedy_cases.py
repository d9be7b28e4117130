"""TEST INFRASTRUCTURE: the fixtures of the greedy-initialisation tests (tests/test_greedy_oracle.py checks their decision margins on the CPU,
tests/test_gpu_init.py runs them on the engine): seeded fp32 videos from synth.make_factors / make_video, the float64 oracle's runs cached per case.

The synthetic seed of every case was found by scanning seeds on the CPU until the oracle's decision margins (tests/greedy_oracle.py) cleared the fixture
bounds below for the automatic search AND for the forced-seed run of the accepted centres.
Case E is synthesised with noise_sd = 3: at the synthesiser's default noise of 1 the background field of so small a field of view (Gaussians 7.5 pixels wide,
fluctuating by 10-30 units) leaks through the 13 x 13 filter and dominates the filtered video, HY / Sn is then several units wide instead of N(0, 1), and the 1.4e6
samples of one 60 x 60 updated box always hold some within 1e-4 Sn of the 3 Sn threshold (2700 seeds scanned, none clean).  With the pixel noise above the leak
the filtered video is what the reference's threshold assumes, and clean seeds turn up at the rate of the other cases."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import greedy_oracle as go
from cnmf_e_amd import synth

# fixture bounds on the oracle's margins: 10 x what tests/test_gpu_seed_images.py asserts of Cn (2e-6 absolute) and PNR (3e-5 relative), 1e-4 for the correlation
# sets, 1e-4 relative for every other comparison
MARGIN_MIN = dict(corr=1e-4, cn=2e-5, pnr=3e-4)
MARGIN_DEFAULT = 1e-4

DECONV = dict(smin=-5.0, optimize_b=True, optimize_pars=True, max_tau=100.0)

#   K = true neurons of the synthetic video; the other keys are the case of the issue
CASES = {
    "A": dict(dims=(44, 40), T=403, K=4, seed=5, gSig=1.5, gSiz=7, pdims=[22, 20], r=5),        # four blocks with halo, T % 4 = 3, per-patch bd, centres kept by patch interior
    "B": dict(dims=(40, 36), T=600, K=1, seed=488, gSig=2.0, gSiz=9, pdims=None, r=8),            # both boxes clipped at every image edge (box2 is 37 x 37 > the block), default bd
    "C": dict(dims=(40, 36), T=600, K=2, seed=130, gSig=2.0, gSiz=9, pdims=None, r=8, nk=3),      # detrended HY and Yw
    "D": dict(dims=(40, 36), T=600, K=2, seed=476, gSig=2.0, gSiz=9, pdims=None, r=8, deconv=True),
    "E": dict(dims=(64, 60), T=400, K=2, seed=497, gSig=3.0, gSiz=16, pdims=None, r=8, noise_sd=3.0),           # tmp_d = 4, 113 taps, an extract box that is not clipped (centre (31, 36))
    "F": dict(dims=(40, 36), T=600, K=3, seed=26, gSig=2.0, gSiz=9, pdims=None, r=8, frame_range=(1, 250), Kmax=2),   # even medians, the cap on K
}
_inputs, _oracle = {}, {}


class _Geometry:
    def create_patch(self, *a):
        pass


def geometry(name):
    from cnmf_e_amd.sources2d import PatchedVideo
    c = CASES[name]
    d1, d2 = c["dims"]
    return PatchedVideo(d1, d2, c["T"], c["pdims"] or [d1, d2], c["r"], _Geometry())


def inputs(name):
    if name not in _inputs:
        c = CASES[name]
        f = synth.make_factors(c["dims"][0], c["dims"][1], c["T"], c["K"], c["seed"], gSig=c["gSig"], gSiz=c["gSiz"], noise_sd=c.get("noise_sd", 1.0))
        Y = synth.make_video(f, np.float32)
        Y.setflags(write=False)
        _inputs[name] = (f, Y)
    return _inputs[name]


def nframes(name):
    fr = CASES[name].get("frame_range")
    return CASES[name]["T"] if fr is None else fr[1]


def oracle(name, forced=False):
    """the oracle's run of a case: the automatic search, or (forced) the forced-seed run of the automatic search's accepted centres.  Computed once, shared."""
    key = (name, forced)
    if key not in _oracle:
        c = CASES[name]
        _, Y = inputs(name)
        kw = dict(nframes=nframes(name), nk=c.get("nk", 1), K=c.get("Kmax"), deconv_opts=DECONV if c.get("deconv") else None)
        seeds = [tuple(int(x) for x in rc) for rc in oracle(name)["center"]] if forced else None
        _oracle[key] = go.greedy_fov(Y, geometry(name), c["gSig"], c["gSiz"], seeds=seeds, **kw)
    return _oracle[key]


def options(name, **extra):
    from cnmf_e_amd.sources2d import Options
    c = CASES[name]
    return Options(ring_radius=c["r"], gSig=c["gSig"], gSiz=c["gSiz"], nk=c.get("nk", 1), deconv_flag=bool(c.get("deconv")), maxIter=3, **extra)
