"""TEST INFRASTRUCTURE: the fixtures of the merge tests (tests/test_merge_oracle.py checks their decision margins on the CPU, tests/test_gpu_merge.py and
tests/test_gpu_merge_mex.py run them on the engine), in the style of tests/residual_cases.py: seeded factors from synth.make_factors at d = 40 x 36 whose
footprints and traces are then edited into the situations a merge must tell apart.  Twelve neurons:

    0        half of a split neuron, trace x0 scaled by 0.6 -- the group's kept member (lowest index) is NOT its strongest trace
    7        the other half (three pixel columns shared), trace x0 + small noise                          -> {0, 7} merge by every criterion
    1, 8, 9  a chain: the footprint of 1 shifted by 2 and by 4 rows; traces x1, x1 + y, y                  -> 1 ~ 8 and 8 ~ 9 but not 1 ~ 9: ONE component {1, 8, 9}
    2, 10    a near miss: 10 is the footprint of 2 shifted by 2 columns with an unrelated trace           -> close, uncorrelated: only merge_close_neighbors takes it
    3        a flat row: C = 2, S = 0 (corr = NaN in its row and column: never merges); its C_raw is 2 + noise, so that the tag ratios stay well defined
             (GetSn of an exactly constant trace is 0 or 1e-17 depending on the rounding of the transform: 0 / 0 against 0 / tiny is no fixture)
    4        a silent neuron: S = 0                                                                        -> tag 2
    5        C_raw == C exactly: std(C_raw - C) = 0, so temp = 0 < 0.1                                     -> tag 4
    6        an ordinary neuron
    11       three pixels                                                                                  -> tag 1 (min_pixel = 5)

C, S and kernel_pars are the float64 oracle's deconvTemporal of the edited raw traces, stored as float32: what a temporal update with deconv_flag leaves.  All
values the product sees are these float32 arrays; the oracle runs in float64 on the same values.

Seeds: for each T the seeds 0, 1, 2, ... were tried on the CPU (test_merge_oracle.py's margin test is the scan's acceptance test) and the first one was kept for which
every decision of every method call in CALLS clears MARGIN (1e-3 absolute on correlations and overlaps), MARGIN_TAG (1 % on the tag ratios) and MARGIN_CUT (1e-4
relative between every difference sample and the 2 sn cut of the S-less branch: the device's GetSn is asserted to 5e-6 of the oracle's by tests/test_gpu_parity.py and
an fp32 difference of fp32 samples is within 6e-8 of the float64 one, so 1e-4 is twenty times what the device can be off; 1 % cannot be asked of 12 x T samples
whose density around the cut is a few per percent).  Distances between argmax pixels are square roots of integers and dmin = 2.5 squared is not an integer.  Both first seeds passed."""
import os
import sys

import numpy as np
import scipy.sparse as sp

HERE = os.path.dirname(os.path.abspath(__file__))
for p_ in (os.path.join(os.path.dirname(HERE), "oracle"), HERE):
    if p_ not in sys.path:
        sys.path.insert(0, p_)

import oasis_oracle as oo
from cnmf_e_amd import synth

D1, D2 = 40, 36
CASES = {"T400": dict(T=400, seed=0), "T403": dict(T=403, seed=0)}              # T % 4 == 0 and T % 4 == 3
MIN_PIXEL = 5
MARGIN = 1e-3
MARGIN_TAG = 1e-2
MARGIN_CUT = 1e-4
DMIN = 2.5
# the method calls every fixture is run through (name -> keyword arguments of the Sources2D method; the oracle functions take the same)
CALLS = {
    "high_corr": ("merge_high_corr", dict(merge_thr=[0.1, 0.5, 0.3])),
    "high_corr_scalar": ("merge_high_corr", dict(merge_thr=0.5)),
    "high_corr_decay": ("merge_high_corr", dict(merge_thr=[0.1, 0.5, 0.3, 5.0])),
    "dist_corr": ("merge_neurons_dist_corr", dict(merge_thr=0.5, dmin=DMIN, method_dist="max")),
    "dist_corr_decay": ("merge_neurons_dist_corr", dict(merge_thr=0.5, dmin=DMIN, method_dist="max", max_decay_diff=5.0)),
    "close": ("merge_close_neighbors", dict(dmin=DMIN, method_dist="max")),
}
_cache = {}


def _shift(col, d1, d2, dr, dc):
    """the footprint (d-vector) moved by (dr, dc) pixels, what leaves the image dropped"""
    img = col.reshape(d1, d2, order="F")
    out = np.zeros_like(img)
    out[max(dr, 0):d1 + min(dr, 0), max(dc, 0):d2 + min(dc, 0)] = img[max(-dr, 0):d1 + min(-dr, 0), max(-dc, 0):d2 + min(-dc, 0)]
    return out.ravel(order="F")


def _ar(rng, T):
    spikes = (rng.random(T) < 0.02) * rng.uniform(5.0, 15.0, T)
    return synth._ar1(spikes, 0.95)


def case(name):
    """dict(d1, d2, T, A (d x 12 csc float32), C, C_raw, S (12 x T float32), kernel_pars (12 float32), video (T x d float32), sn)"""
    if name in _cache:
        return _cache[name]
    c = CASES[name]
    T = c["T"]
    f = synth.make_factors(D1, D2, T, 7, c["seed"], gSig=2.0, gSiz=9, min_sep=9)
    rng = np.random.default_rng(1000 + c["seed"])
    A0 = np.asarray(f.A_true.todense(), dtype=np.float64)
    d = D1 * D2
    A = np.zeros((d, 12))
    A[:, :7] = A0
    X = np.stack([_ar(rng, T) for _ in range(7)])                                # traces with enough events at T = 400 (synth's own rate leaves some rows nearly empty)
    y, z, w = _ar(rng, T), _ar(rng, T), _ar(rng, T)
    noise = lambda s=0.3: rng.normal(0.0, s, T)
    R = np.zeros((12, T))
    for k in range(7):
        R[k] = X[k] + noise()
    # the split pair: two overlapping halves of footprint 0
    img = A0[:, 0].reshape(D1, D2, order="F")
    cc = int(np.argmax(img.max(axis=0)))
    left, right = img.copy(), img.copy()
    left[:, cc + 2:] = 0; right[:, :cc - 1] = 0
    A[:, 0] = left.ravel(order="F"); A[:, 7] = right.ravel(order="F")
    R[0] = 0.6 * (X[0] + noise(0.1)); R[7] = X[0] + noise(0.1)
    # the chain
    A[:, 8] = _shift(A0[:, 1], D1, D2, 2, 0); A[:, 9] = _shift(A0[:, 1], D1, D2, 4, 0)
    R[1] = X[1] + noise(); R[8] = X[1] + y + noise(); R[9] = y + noise()
    # the near miss
    A[:, 10] = _shift(A0[:, 2], D1, D2, 0, 2); R[10] = z + noise()
    # three pixels in a corner
    A[[0, 1, 2], 11] = [1.0, 0.8, 0.6]; R[11] = w + noise()
    R += 0.7                                                                    # a baseline for the deconvolution to find
    R32 = R.astype(np.float32)
    Cd, Rd, Sd, kp, sn = oo.deconvTemporal(R32.astype(np.float64))
    C = Cd.astype(np.float32); Craw = Rd.astype(np.float32); S = Sd.astype(np.float32); kp = np.asarray(kp, dtype=np.float32)
    C[3] = 2.0; Craw[3] = (2.0 + rng.normal(0.0, 0.3, T)).astype(np.float32); S[3] = 0.0; kp[3] = 0.0      # flat
    S[4] = 0.0                                                                  # silent
    Craw[5] = C[5]                                                              # C_raw == C
    Y = synth.make_video(f, np.float32)
    out = dict(d1=D1, d2=D2, T=T, A=sp.csc_matrix(A.astype(np.float32)), C=C, C_raw=Craw, S=S, kernel_pars=kp, video=Y, sn=f.sn, factors=f)
    for v in (C, Craw, S, kp):
        v.setflags(write=False)
    _cache[name] = out
    return out


def traces(K, T, seed=5):
    """K x T float32 rows of unit scale for the correlation / Gram checks (K = 0, 1, 15, 16, 17, 33: the edges of the 16 x 16 tiles); from K = 15 on the row
    K - 2 is constant (the NaN path) and rows 0, 1 are nearly equal"""
    rng = np.random.default_rng(seed + 31 * K + T)
    X = rng.normal(0.0, 1.0, (K, T))
    if K:
        X += rng.normal(0.0, 0.5, (K, 1))                                       # means that matter: the centring is part of what is checked
    if K >= 2:
        X[1] = X[0] + 0.05 * rng.normal(0.0, 1.0, T)
    if K >= 15:
        X[K - 2] = 1.25
    return np.ascontiguousarray(X, dtype=np.float32)


def oracle_call(name, call):
    """the float64 oracle's result of CALLS[call] on fixture `name` (cached)"""
    key = (name, call)
    if key not in _cache:
        import merge_oracle as mo
        c = case(name)
        meth, kw = CALLS[call]
        args = (c["A"], c["C"], c["C_raw"], c["S"], c["kernel_pars"])
        if meth == "merge_high_corr":
            _cache[key] = mo.merge_high_corr(*args, kw["merge_thr"])
        elif meth == "merge_neurons_dist_corr":
            _cache[key] = mo.merge_neurons_dist_corr(*args, c["d1"], c["d2"], kw["merge_thr"], kw["dmin"], kw["method_dist"], kw.get("max_decay_diff"))
        else:
            _cache[key] = mo.merge_close_neighbors(*args, c["d1"], c["d2"], kw["dmin"], kw["method_dist"])
    return _cache[key]
