"""Greedy initialisation on the device: Sources2D.initComponents_parallel (cnmfe_peel_open / _extract / _apply / _close, csrc/peel.hpp; the search loop in
hostops.greedy_roi_block) against the float64 oracle tests/greedy_oracle.py on the seeded fp32 videos of tests/greedy_cases.py.

The discrete decisions -- the pixel sets {corr > 0.9} and {corr < 0.3}, the entries a threshold zeroes, the list of centres and its order -- must be EQUAL to the
oracle's: tests/test_greedy_oracle.py::test_fixture_margins shows that every one of them is decided by a margin far above fp32 rounding on these fixtures.
The continuous quantities are compared relative to the oracle's max |ci|, max |ai|, ... (PNR: per entry; Cn: absolute).

Bounds: the rule of tests/test_gpu_parity.py -- 10 x the error observed on the MI355X against this oracle, rounded up to one digit, never above 1e-4.  Observed on
the MI355X (worst over the cases A-F, recorded per case through the `observed` fixture):
    steps (forced seeds)   ci / max|ci|   ai / max|ai|   PNR relative   Cn absolute
        A                  8.1e-8         1.3e-6         2.7e-6         3.3e-7
        B                  6.8e-8         1.6e-7         9.9e-7         6.3e-8
        C                  1.0e-7         5.6e-8         8.2e-7         1.3e-7
        D                  1.3e-7         2.7e-7         8.7e-7         8.6e-8
        E                  1.2e-7         1.7e-6         5.0e-7         5.2e-7
        F                  1.1e-7         2.3e-6         1.5e-6         2.1e-7
    end to end: A / max|A| 1.8e-6 (E), C / max|C| 1.2e-7 (E), C_raw 1.2e-7 (D); case D: C 5.9e-8, C_raw 9.8e-8, S 8.3e-8 (Frobenius), gamma 2.6e-8
The worst case sets each bound: ci 1.3e-7 -> 2e-6, ai 2.3e-6 -> 3e-5, PNR 2.7e-6 -> 3e-5, Cn 5.2e-7 -> 6e-6, A 1.8e-6 -> 2e-5, C and C_raw 1.2e-7 -> 2e-6.
The deconvolved quantities of case D use the bounds test_hals_temporal_deconv_parity asserts (traces 5e-6 relative, gamma 2e-6 absolute)."""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import greedy_cases as gc
from parity_util import rel

pytestmark = pytest.mark.gpu

CI_TOL = 2e-6         # max |ci - ci_o| / max |ci_o| after every extract
AI_TOL = 3e-5         # max |ai - ai_o| / max |ai_o| after every extract (before the constraints)
PNR_TOL = 3e-5        # relative, per entry of the updated box
CN_TOL = 6e-6         # absolute, per entry of the updated box
A_TOL = 2e-5          # max |A - A_o| / max |A_o|
C_TOL = 2e-6          # max |C - C_o| / max |C_o|, likewise C_raw
DECONV_TOL = 5e-6     # test_hals_temporal_deconv_parity: relative Frobenius error of C, C_raw (and S)
GAMMA_TOL = 2e-6      # ... and the absolute error of the AR(1) coefficient

_runs = {}


def _run(name, forced=False, lanes=1, steps=False):
    """initComponents_parallel of a case on a fresh engine -> dict(center, Cn, PNR, A, C, C_raw, S, kernel_pars, images (correlation_pnr_parallel), steps)"""
    from cnmf_e_amd.engine import Engine
    from cnmf_e_amd.sources2d import PatchedVideo, Sources2D
    c = gc.CASES[name]
    f, Y = gc.inputs(name)
    d1, d2 = c["dims"]
    eng = Engine(0)
    try:
        if lanes != 1:
            eng.set_option("lanes", lanes)
        video = PatchedVideo(d1, d2, c["T"], c["pdims"] or [d1, d2], c["r"], eng)
        video.upload_from_full(Y)
        s = Sources2D(video, gc.options(name), f.A_init, f.C_init, f.sn)
        log = {}
        if steps:
            s._init_observer = lambda idx, kind, data: log.setdefault(idx, []).append((kind, data))
        seeds = [tuple(int(x) for x in rc) for rc in gc.oracle(name)["center"]] if forced else None
        center, Cn, PNR = s.initComponents_parallel(K=c.get("Kmax"), frame_range=c.get("frame_range"), seeds=seeds)
        out = dict(center=center, Cn=Cn, PNR=PNR, A=s.A.toarray().astype(np.float64), C=np.asarray(s.C, dtype=np.float64), C_raw=np.asarray(s.C_raw, dtype=np.float64),
                   S=np.asarray(s.S, dtype=np.float64), kernel_pars=s.P.get("kernel_pars"), steps=log, ids=s.ids)
        out["images"] = s.correlation_pnr_parallel(c.get("frame_range"))
        return out
    finally:
        eng.close()


def _cached(name, forced=False):
    key = (name, forced)
    if key not in _runs:
        _runs[key] = _run(name, forced, steps=forced)
    return _runs[key]


def _maxrel(a, b):
    return float(np.max(np.abs(np.asarray(a) - np.asarray(b))) / np.max(np.abs(b)))


@pytest.mark.parametrize("name", list(gc.CASES))
def test_step_parity_under_forced_seeds(name, observed):
    """the oracle's accepted centres forced as seeds: after every extract the two correlation sets are the oracle's and ci, ai are within tolerance; after
    every apply the PNR and Cn boxes are, and the entries a threshold zeroed are zero in both"""
    got = _cached(name, True)
    ora = gc.oracle(name, True)
    e = dict(ci=0.0, ai=0.0, pnr=0.0, cn=0.0)
    nsteps = 0
    for idx, blk in ora["blocks"].items():
        mine = got["steps"].get(idx, [])
        assert [k for k, _ in mine] == [s["kind"] for s in blk["steps"]], (idx, [k for k, _ in mine], [s["kind"] for s in blk["steps"]])
        for (kind, d), o in zip(mine, blk["steps"]):
            assert (d["r"], d["c"]) == (o["r"], o["c"])
            nsteps += 1
            if kind == "extract":
                with np.errstate(invalid="ignore"):
                    assert np.array_equal(d["corr"] > 0.9, o["hi"]) and np.array_equal(d["corr"] < 0.3, o["lo"]), (idx, d["r"], d["c"])
                assert d["stats"]["n_hi"] == int(o["hi"].sum()) and d["stats"]["n_lo"] == int(o["lo"].sum())
                e["ci"] = max(e["ci"], _maxrel(d["ci"], o["ci"]))
                if o["ai"] is not None:
                    e["ai"] = max(e["ai"], _maxrel(d["ai"], o["ai"]))
            else:
                assert np.array_equal(d["pnr"] == 0, o["pnr"] == 0) and np.array_equal(d["cn"] == 0, o["cn"] == 0), (idx, d["r"], d["c"])
                nz = o["pnr"] != 0
                if nz.any():
                    e["pnr"] = max(e["pnr"], float(np.max(np.abs(d["pnr"] - o["pnr"])[nz] / o["pnr"][nz])))
                e["cn"] = max(e["cn"], float(np.max(np.abs(d["cn"] - o["cn"]))))
    observed["init_steps_%s" % name] = e
    print("init steps %s: %d steps  ci %.3e  ai %.3e  PNR rel %.3e  Cn abs %.3e" % (name, nsteps, e["ci"], e["ai"], e["pnr"], e["cn"]))
    assert nsteps >= 2
    assert e["ci"] <= CI_TOL and e["ai"] <= AI_TOL and e["pnr"] <= PNR_TOL and e["cn"] <= CN_TOL, e


@pytest.mark.parametrize("name", list(gc.CASES))
def test_end_to_end_automatic_search(name, observed):
    got = _cached(name)
    ora = gc.oracle(name)
    c = gc.CASES[name]
    assert np.array_equal(got["center"], ora["center"]), (got["center"], ora["center"])
    K = ora["center"].shape[0]
    assert K >= 1 and got["A"].shape == ora["A"].shape and got["C"].shape == (K, gc.nframes(name))
    assert np.array_equal(got["ids"], np.arange(1, K + 1))
    e = dict(A=_maxrel(got["A"], ora["A"]), C=_maxrel(got["C"], ora["C"]), C_raw=_maxrel(got["C_raw"], ora["C_raw"]))
    if c.get("deconv"):
        e["C_fro"] = max(rel(got["C"][k], ora["C"][k]) for k in range(K))
        e["C_raw_fro"] = max(rel(got["C_raw"][k], ora["C_raw"][k]) for k in range(K))
        e["S_fro"] = max(rel(got["S"][k], ora["S"][k]) for k in range(K))
        e["gamma"] = float(np.max(np.abs(np.asarray(got["kernel_pars"], dtype=np.float64) - np.asarray(ora["kernel_pars"], dtype=np.float64))))
    observed["init_e2e_%s" % name] = e
    print("init e2e %s: K %d  %s" % (name, K, {k: "%.3e" % v for k, v in e.items()}))
    assert np.array_equal(got["A"] != 0, ora["A"] != 0)
    if c.get("deconv"):
        assert e["A"] <= A_TOL
        assert e["C_fro"] <= DECONV_TOL and e["C_raw_fro"] <= DECONV_TOL and e["S_fro"] <= DECONV_TOL and e["gamma"] <= GAMMA_TOL, e
    else:
        assert e["A"] <= A_TOL and e["C"] <= C_TOL and e["C_raw"] <= C_TOL, e
        assert not got["S"].any()
    # the images returned are the seed images of the same object, bit for bit
    assert np.array_equal(got["Cn"], got["images"][0]) and np.array_equal(got["PNR"], got["images"][1])


def test_two_runs_and_two_lanes_are_bit_identical():
    a, b, l2 = _cached("A"), _run("A"), _run("A", lanes=2)
    for other in (b, l2):
        assert np.array_equal(a["center"], other["center"]) and np.array_equal(a["A"], other["A"]) and np.array_equal(a["C"], other["C"])


def _iteration(with_init, from_init=False):
    from cnmf_e_amd.engine import Engine
    from cnmf_e_amd.sources2d import PatchedVideo, Sources2D
    c = gc.CASES["A"]
    f, Y = gc.inputs("A")
    d1, d2 = c["dims"]
    eng = Engine(0)
    try:
        video = PatchedVideo(d1, d2, c["T"], c["pdims"], c["r"], eng)
        video.upload_from_full(Y)
        s = Sources2D(video, gc.options("A"), f.A_init, f.C_init, f.sn)
        if with_init:
            s.initComponents_parallel()
            if not from_init:
                s.set_components(f.A_init, f.C_init)
        s.update_background_parallel()
        W = [s.get_W(idx).data.copy() for idx in video.owned]
        s.update_spatial_parallel()
        A = s.A.toarray()
        s.update_temporal_parallel()
        return W, A, np.asarray(s.C, dtype=np.float32).copy()
    finally:
        eng.close()


def test_an_iteration_after_the_initialisation_is_unchanged():
    W0, A0, C0 = _iteration(False)
    W1, A1, C1 = _iteration(True)
    assert all(np.array_equal(a, b) for a, b in zip(W0, W1))
    assert np.array_equal(A0, A1) and np.array_equal(C0, C1)


def test_an_iteration_from_the_initialisation_runs():
    W, A, C = _iteration(True, from_init=True)
    assert all(np.all(np.isfinite(w)) for w in W) and np.all(np.isfinite(A)) and np.all(np.isfinite(C))
    assert A.shape[1] == gc.oracle("A")["center"].shape[0] and A.any() and C.any()


def _small_engine(Y, d1, d2, T, r=3):
    from cnmf_e_amd.engine import Engine
    from cnmf_e_amd.sources2d import PatchedVideo
    eng = Engine(0)
    video = PatchedVideo(d1, d2, T, [d1, d2], r, eng)
    video.upload_from_full(Y)
    return eng, video


def test_edges_return_codes_or_no_success():
    from cnmf_e_amd import hostops, synth
    from cnmf_e_amd._lib import CnmfeError
    from cnmf_e_amd.sources2d import Sources2D, Options, seed_psf
    # a 12 x 12 block with gSiz 7: the box covers the block; the background set may be empty -> ai = 0, y_bg = NaN, never a fault
    d1, d2, T = 12, 12, 120
    f = synth.make_factors(d1, d2, T, 1, 2, gSig=1.5, gSiz=7, min_sep=3)
    Y = synth.make_video(f, np.float32).copy()
    Y[:, 5 * d1 + 4] = 7.0                                               # one constant pixel
    eng, video = _small_engine(Y, d1, d2, T)
    try:
        with pytest.raises(CnmfeError, match="error -4"):
            eng.peel_extract(0, 5, 5, 7)                                 # no session
        with pytest.raises(CnmfeError, match="error -4"):
            eng.peel_close(0)
        Cn, PNR, Sn = eng.peel_open(0, seed_psf(1.5, 7, True))
        with pytest.raises(CnmfeError, match="error -4"):
            eng.peel_open(0, seed_psf(1.5, 7, True))                     # a second open
        with pytest.raises(CnmfeError, match="error -5"):
            eng.peel_extract(0, 5, 5, 21)
        with pytest.raises(CnmfeError, match="error -1"):
            eng.peel_extract(0, 12, 5, 7)
        for (r, c) in ((6, 6), (0, 0), (11, 11), (4, 5)):               # centre, two corners, the constant pixel
            corr, ai, ci, st = eng.peel_extract(0, r, c, 7)
            r0, r1, c0, c1 = hostops.box_of(d1, d2, r, c, 7)
            assert corr.shape == (r1 - r0, c1 - c0) and ai.shape == corr.shape and np.all(ai >= 0) and np.all(np.isfinite(ai))
            assert st["n_lo"] == int(np.sum(corr < 0.3)) and (st["n_lo"] > 0 or not ai.any())
            assert abs(corr[r - r0, c - c0] - 1.0) < 1e-12
            big = np.zeros((d1, d2)); big[r0:r1, c0:c1] = ai
            pnr, cn = eng.peel_apply(0, r, c, 7, ai, big, np.nan_to_num(ci), 3.0, 5.0, 0.15)
            assert pnr.shape == (d1, d2) and np.all(np.isfinite(pnr)) and np.all(np.isfinite(cn)) and np.all(cn <= 1.0)
        eng.peel_close(0)
        Cn2, PNR2 = eng.seed_images(0, seed_psf(1.5, 7, True))           # open returned the seed images, and the resident video is untouched
        assert np.array_equal(Cn, Cn2) and np.array_equal(PNR, PNR2)
        # no filter: the constant pixel has Sn = 0, its trace is constant -> corr = NaN everywhere, both sets empty, "no success"
        Cn, PNR, Sn = eng.peel_open(0, None)
        assert Sn[5 * d1 + 4] == 0
        corr, ai, ci, st = eng.peel_extract(0, 4, 5, 7)
        assert np.all(np.isnan(corr)) and st["n_hi"] == 0 and st["n_lo"] == 0 and not ai.any()
        eng.peel_close(0)
        # the whole method on this block: runs, finds at most a neuron, returns finite images apart from the constant pixel
        s = Sources2D(video, Options(ring_radius=3, gSig=1.5, gSiz=7, min_pnr=5.0), f.A_init, f.C_init, f.sn)
        center, Cn, PNR = s.initComponents_parallel()
        assert center.shape[1] == 2 and s.A.shape[1] == center.shape[0] == s.C.shape[0]
        for bad in (dict(ssub=2), dict(tsub=2), dict(nk=3, detrend_method="local_min")):
            s.options = Options(ring_radius=3, gSig=1.5, gSiz=7, **bad)
            with pytest.raises(NotImplementedError):
                s.initComponents_parallel()
        s.options = Options(ring_radius=3, gSig=1.5, gSiz=7)
        for kw in (dict(frame_range=(5, 100)), dict(use_prev=True), dict(save_avi=True), dict(debug_on=True)):
            with pytest.raises(NotImplementedError):
                s.initComponents_parallel(**kw)
        eng.peel_open(0, None); eng.peel_close(0)                        # ... and no refused or finished call left a session behind
    finally:
        eng.close()
