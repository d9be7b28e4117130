"""TEST INFRASTRUCTURE: the fixtures of the second initialisation pass under background_model = 'svd' (tests/test_svd_second_pass_host.py checks their decision
margins on the CPU, tests/test_gpu_svd_second_pass.py runs them on the engine).  The recordings are those of tests/svd_bg_cases.py (make_case); the model
(A0, C0) keeps the neurons `keep` and WITHHOLDS the others, one background update fits b, f, b0 (tests/svd_bg_oracle.py), and the float64 oracle's second pass runs
per patch on
    Yres = Y(patch) - A0(patch, :) C0 - (b f + b0)        (@Sources2D/initComponents_residual_parallel.m:107-122,195-199,224-227: the session's block is the patch)
through tests/greedy_oracle.py::greedy_block, collected like tests/residual_cases.py::collect.

(shape, nb, keep, seed) of every case was chosen on the CPU in the way of scripts/residual_seed_scan.py: the oracle's decision margins clear the bounds of
tests/greedy_cases.py (MARGIN_MIN / MARGIN_DEFAULT) for the automatic search, and every withheld neuron is found.  `one` with nb = 1, seed 0 does not (its
smallest margin is 6.2e-5 < MARGIN_DEFAULT), which is why `one` runs with nb = 3.  Smallest margins of the chosen cases: one pnr 1.0e-3, hy 2.6e-4; small pnr
1.7e-3, hy 1.0e-3; quad pnr 6.5e-4, hy 2.5e-3; one_d hy 2.4e-4."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import residual_cases as rc
import svd_bg_cases as sc
import svd_bg_oracle as so

GSIG, GSIZ, MIN_CORR, MIN_PNR = 1.5, 7, 0.5, 4.0
#   keep: the neurons of svd_bg_cases.SHAPES[shape]["centres"] the model knows; the others are what the second pass has to find
CASES = {
    "one": dict(shape="one", nb=3, keep=[0, 2, 4], seed=0),                    # one patch, T mod 4 = 3, d no multiple of 256
    "small": dict(shape="small", nb=1, keep=[0], seed=0),                      # d < T
    "quad": dict(shape="quad", nb=2, keep=[0, 1, 2], seed=0),                  # 2 x 2 patches: a kept neuron straddles a patch border, two patches hold no neuron
    "one_d": dict(shape="one", nb=3, keep=[0, 2, 4], seed=0, deconv=True),     # deconv_flag: S and kernel_pars grow
}
_inputs, _loop, _oracle = {}, {}, {}


def case(name):
    """the case as tests/residual_cases.py::collect reads it (dims, T, gSig, gSiz, min_corr, min_pnr, deconv)"""
    c = dict(CASES[name])
    s = sc.SHAPES[c["shape"]]
    c.update(dims=(s["d1"], s["d2"]), T=s["T"], patch=s["patch"], halo=s["halo"], gSig=GSIG, gSiz=GSIZ, min_corr=MIN_CORR, min_pnr=MIN_PNR,
             withheld=[k for k in range(len(s["centres"])) if k not in c["keep"]])
    return c


def inputs(name):
    """(recording of svd_bg_cases.make_case with ALL neurons in the video, A0 (d x len(keep) csc float32), C0): the model of the kept neurons"""
    if name not in _inputs:
        c = CASES[name]
        rec = sc.make_case(c["shape"], c["nb"], True, seed=c["seed"])
        rec["Y"].setflags(write=False)
        _inputs[name] = (rec, rec["A"][:, c["keep"]].tocsc(), np.ascontiguousarray(rec["C"][c["keep"]]))
    return _inputs[name]


def oracle_loop(name):
    """the float64 oracle object of the case after one update_background_parallel (computed once; do not modify)"""
    if name not in _loop:
        c = case(name)
        rec, A0, C0 = inputs(name)
        d1, d2 = c["dims"]
        o = so.SvdOracleLoop(rec["Y"].T.astype(np.float64).reshape(d1, d2, c["T"], order="F"), d1, d2, c["T"], c["patch"], c["halo"], A0, C0, nb=c["nb"], maxIter=5)
        o.update_background_parallel()
        _loop[name] = o
    return _loop[name]


def yres(o, idx, b=None, f=None, b0=None):
    """Yres of a patch in float64: Y(patch) - A(patch, :) C - (b f + b0); b, f, b0 default to the oracle's own fit"""
    b = o.b[idx] if b is None else b; f = o.f[idx] if f is None else f; b0 = o.b0[idx] if b0 is None else b0
    mp = o._mask(o.patch_pos[idx])
    return o._data(o.patch_pos[idx]) - o.A.tocsr()[mp] @ o.C - (b @ f + b0[:, None])


def collect(name, source, seeds=None):
    return rc.collect(case(name), oracle_loop(name), source, seeds)


def oracle(name):
    """the oracle's second pass (automatic search) of a case on ITS OWN Yres.  Computed once."""
    if name not in _oracle:
        o = oracle_loop(name)
        _oracle[name] = collect(name, lambda idx: yres(o, idx))
    return _oracle[name]


def true_centres(name):
    """the withheld neurons' centres as 1-based FOV pixels (row, column), rounded"""
    c = case(name)
    ctr = np.asarray(sc.SHAPES[c["shape"]]["centres"])[c["withheld"]]
    return np.floor(ctr).astype(np.int64) + 1


def options(name, **extra):
    from cnmf_e_amd.sources2d import Options
    c = case(name)
    kw = dict(ring_radius=c["halo"], background_model="svd", nb=c["nb"], gSig=GSIG, gSiz=GSIZ, deconv_flag=bool(c.get("deconv")), maxIter=5, bd=rc.BD)
    kw.update(extra)
    return Options(**kw)
