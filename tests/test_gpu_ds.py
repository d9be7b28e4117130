"""The down-sampled seed images and first initialisation on the device (options.ssub / options.tsub: cnmfe_seed_images_ds, cnmfe_peel_open_ds, csrc/ds.hpp --
k_ds_video, k_ds_coef; the rescaling and the way back to full resolution in sources2d / hostops) against the float64 oracle tests/ds_oracle.py on the seeded
fp32 videos of tests/ds_cases.py.

What is compared.
  Yds_out   the fp32 video a session searches against dsData(detrended block) of the oracle (the centred video: the oracle's minus box(fp32 pixel mean), which
            is what the resident video lacks), max |.| relative to max |Yds|, cases P-S.
  identity  ssub = tsub = 1: Yds_out is the centred video bit for bit, the images are peel_open's.
  images    correlation_pnr_parallel: PNR on every pixel (relative), Cn on the robust pixels (absolute) -- the fragile-pixel rule of test_gpu_seed_images.py
            evaluated on the low-resolution grid before the resize; a full-resolution pixel is left out when any low-resolution pixel it is interpolated from
            is fragile or has a fragile 8-neighbour.  At most 10 % of a case may be left out; the oracle alone leaves out 0.0 % (P), 0.0 % (Q), 0.0 % (R),
            0.0 % (S), 0.0 % (U).
  init      step parity under forced seeds (the sets and the zeroed entries EQUAL the oracle's: tests/test_ds_oracle.py::test_fixture_margins; ci, ai, PNR, Cn
            within tolerance) and the end-to-end result (center equal; A, C, C_raw within tolerance, for U also S and gamma).

Bounds: the rule of tests/test_gpu_parity.py -- 10 x the error observed on the MI355X against this oracle, rounded up to one digit, never above 1e-4.  Observed on
the MI355X (recorded per case through the `observed` fixture):
    Yds_out            P 0 (exact: eight exact fp32 differences, their mean fits 24 bits)   Q 5.3e-8   R 3.1e-8   S 4.2e-8
    images             PNR relative / Cn absolute (robust = all pixels):  P 1.1e-6 / 1.4e-7   Q 1.6e-6 / 4.0e-8   R 2.4e-6 / 1.9e-7   S 1.9e-6 / 1.6e-7   U 1.3e-6 / 1.6e-7
    steps              ci / max|ci|   ai / max|ai|   PNR relative   Cn absolute
        P              1.2e-7         9.0e-7         1.3e-6         2.0e-7
        Q              2.0e-7         6.1e-6         2.4e-5         5.5e-7
        R              1.3e-7         1.7e-6         2.9e-6         1.1e-6
        S              8.2e-8         4.0e-8         9.1e-7         9.5e-8
        U              3.8e-7         3.3e-6         4.0e-6         5.3e-7
    end to end         A / max|A| 5.6e-6 (Q), C and C_raw / max 1.2e-7 (Q); U: C 3.0e-7, C_raw 3.1e-7, S 3.5e-7 (relative Frobenius, per neuron), gamma 2.9e-8
The worst case sets each bound: Yds 5.3e-8 -> 6e-7; images PNR 2.4e-6 -> 3e-5, Cn 1.9e-7 -> 2e-6; steps ci 3.8e-7 -> 4e-6, ai 6.1e-6 -> 7e-5, PNR 2.4e-5 -> the cap
1e-4 (case Q: a 15 x 13 grid whose updated box is the whole image, the entries just above min_pnr / 2), Cn 1.1e-6 -> 2e-5; A 5.6e-6 -> 6e-5, C and C_raw 1.2e-7 ->
2e-6; U: traces 3.5e-7 -> 4e-6, gamma 2.9e-8 -> 3e-7."""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import ds_cases as dc
import ds_oracle as dso
from parity_util import rel

pytestmark = pytest.mark.gpu

YDS_TOL = 6e-7        # max |Yds - Yds_o| / max |Yds_o|
PNR_IMG_TOL = 3e-5    # correlation_pnr_parallel: relative, every pixel
CN_IMG_TOL = 2e-6     # ... absolute, robust pixels
CI_TOL = 4e-6         # steps: max |ci - ci_o| / max |ci_o|
AI_TOL = 7e-5         # steps: max |ai - ai_o| / max |ai_o| (before the constraints)
PNR_TOL = 1e-4        # steps: relative, per entry of the updated box (10 x 2.4e-5 is above the cap)
CN_TOL = 2e-5         # steps: absolute, per entry of the updated box
A_TOL = 6e-5          # max |A - A_o| / max |A_o|
C_TOL = 2e-6          # max |C - C_o| / max |C_o|, likewise C_raw
DECONV_TOL = 4e-6     # case U: relative Frobenius error of C, C_raw and S per neuron ...
GAMMA_TOL = 3e-7      # ... and the absolute error of the AR(1) coefficient
MAX_LEFT_OUT = 0.10

_runs, _imgs = {}, {}


def _sources(name, eng, lanes=1):
    from cnmf_e_amd.sources2d import PatchedVideo, Sources2D
    c = dc.CASES[name]
    f, Y = dc.inputs(name)
    d1, d2 = c["dims"]
    if lanes != 1:
        eng.set_option("lanes", lanes)
    video = PatchedVideo(d1, d2, c["T"], c["pdims"] or [d1, d2], c["r"], eng)
    video.upload_from_full(Y)
    return video, Sources2D(video, dc.options(name), f.A_init, f.C_init, f.sn)


def _run(name, forced=False, lanes=1):
    """initComponents_parallel of a case on a fresh engine"""
    from cnmf_e_amd.engine import Engine
    eng = Engine(0)
    try:
        video, s = _sources(name, eng, lanes)
        log, opened = {}, {}

        def observer(idx, kind, data):
            if kind == "open":
                opened[idx] = dict(data, ymean=eng.ymean(video.pid[idx]))
            else:
                log.setdefault(idx, []).append((kind, data))
        if forced:
            s._init_observer = observer
        seeds = [tuple(int(x) for x in rc) for rc in dc.oracle(name)["center"]] if forced else None
        center, Cn, PNR = s.initComponents_parallel(seeds=seeds)
        return dict(center=center, Cn=Cn, PNR=PNR, A=s.A.toarray().astype(np.float64), C=np.asarray(s.C, dtype=np.float64), C_raw=np.asarray(s.C_raw, dtype=np.float64),
                    S=np.asarray(s.S, dtype=np.float64), kernel_pars=s.P.get("kernel_pars"), steps=log, opened=opened, ids=s.ids)
    finally:
        eng.close()


def _cached(name, forced=False):
    key = (name, forced)
    if key not in _runs:
        _runs[key] = _run(name, forced)
    return _runs[key]


def _images(name, lanes=1, calls=1):
    from cnmf_e_amd.engine import Engine
    eng = Engine(0)
    try:
        _video, s = _sources(name, eng, lanes)
        return [s.correlation_pnr_parallel() for _ in range(calls)]
    finally:
        eng.close()


def _cached_images(name):
    if name not in _imgs:
        _imgs[name] = _images(name, calls=2)
    return _imgs[name]


def _maxrel(a, b):
    return float(np.max(np.abs(np.asarray(a) - np.asarray(b))) / np.max(np.abs(b)))


@pytest.mark.parametrize("name", ["P", "Q", "R", "S"])
def test_yds_out_against_the_oracle(name, observed):
    c = dc.CASES[name]
    _, Y = dc.inputs(name)
    geo = dc.geometry(name)
    got = _cached(name, True)["opened"]
    assert set(got) == set(geo.order)
    worst = 0.0
    for idx in geo.order:
        bp = [int(x) for x in geo.block_pos[idx]]
        nr, nc = bp[1] - bp[0] + 1, bp[3] - bp[2] + 1
        Yb = np.asarray(Y[:, geo.block_pix[idx]], dtype=np.float64).T
        ref, d1s, d2s = dso.peel_video(Yb, nr, nc, c.get("nk", 1), c["ssub"], c["tsub"])
        if c.get("nk", 1) == 1:                                            # the resident video is Y - fp32(mean): the session's video lacks box(that mean)
            m = got[idx]["ymean"].astype(np.float32).astype(np.float64).reshape(nr, nc, order="F")
            ref = ref - (dso.imresize(m, (d1s, d2s), "box") if c["ssub"] > 1 else m).reshape(-1, 1, order="F")
        yds = got[idx]["Yds"]
        assert yds.dtype == np.float32 and yds.shape == (c["T"] // c["tsub"], d1s * d2s)
        worst = max(worst, _maxrel(yds.T.astype(np.float64), ref))
    observed["ds_yds_%s" % name] = worst
    print("ds Yds_out %s: %.3e" % (name, worst))
    assert worst <= YDS_TOL, worst


def test_identity_is_bit_identical_to_peel_open():
    from cnmf_e_amd.engine import Engine
    from cnmf_e_amd.sources2d import PatchedVideo, seed_psf
    c = dc.CASES["R"]
    _, Y = dc.inputs("R")
    d1, d2 = c["dims"]
    n = 403                                                                # fewer frames than the recording, n % 4 = 3
    eng = Engine(0)
    try:
        video = PatchedVideo(d1, d2, c["T"], [d1, d2], c["r"], eng)
        video.upload_from_full(Y)
        psf = seed_psf(c["gSig"], c["gSiz"], True)
        ref = eng.peel_open(0, psf, n, None, 3.0)
        ex_ref = eng.peel_extract(0, 20, 18, 9)
        eng.peel_close(0)
        cn, pnr, sn, yds = eng.peel_open_ds(0, 1, 1, psf, n, None, 3.0, want_video=True)
        ex = eng.peel_extract(0, 20, 18, 9)
        eng.peel_close(0)
        assert np.array_equal(cn, ref[0]) and np.array_equal(pnr, ref[1]) and np.array_equal(sn, ref[2])
        centred = Y[:n] - eng.ymean(0).astype(np.float32)[None, :]         # k_center4: the fp32 difference of the sample and the fp32 mean
        assert yds.shape == (n, d1 * d2) and np.array_equal(yds, centred)
        for a, b in zip(ex[:3], ex_ref[:3]):
            assert np.array_equal(a, b, equal_nan=True)
        assert ex[3] == ex_ref[3]
    finally:
        eng.close()


@pytest.mark.parametrize("name", list(dc.CASES))
def test_correlation_pnr_parallel_parity(name, observed):
    Cn, PNR = _cached_images(name)[0]
    Cn_o, PNR_o, robust = dc.oracle_images(name)
    d1, d2 = dc.CASES[name]["dims"]
    assert Cn.shape == (d1, d2) and PNR.shape == (d1, d2) and Cn.dtype == np.float64
    assert np.all(np.isfinite(Cn)) and np.all(np.isfinite(PNR))
    e_pnr = float(np.max(np.abs(PNR - PNR_o) / np.abs(PNR_o)))
    e_cn = float(np.max(np.abs(Cn - Cn_o)[robust]))
    left = float((~robust).mean())
    observed["ds_images_%s" % name] = dict(pnr_rel=e_pnr, cn_abs_robust=e_cn, cn_abs_all=float(np.max(np.abs(Cn - Cn_o))), left_out=left)
    print("ds seed images %s: PNR rel %.3e  Cn abs (robust) %.3e  left out %.2f %%" % (name, e_pnr, e_cn, 100 * left))
    assert left <= MAX_LEFT_OUT, left
    assert e_pnr <= PNR_IMG_TOL, e_pnr
    assert e_cn <= CN_IMG_TOL, e_cn


@pytest.mark.parametrize("name", list(dc.CASES))
def test_step_parity_under_forced_seeds(name, observed):
    """the oracle's accepted centres forced as seeds: on the LOW-RESOLUTION grid, after every extract the two correlation sets are the oracle's and ci, ai are
    within tolerance; after every apply the PNR and Cn boxes are, and the entries a threshold zeroed are zero in both"""
    got = _cached(name, True)
    ora = dc.oracle(name, True)
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
    observed["ds_steps_%s" % name] = e
    print("ds init steps %s: %d steps  ci %.3e  ai %.3e  PNR rel %.3e  Cn abs %.3e" % (name, nsteps, e["ci"], e["ai"], e["pnr"], e["cn"]))
    assert nsteps >= 2
    assert e["ci"] <= CI_TOL and e["ai"] <= AI_TOL and e["pnr"] <= PNR_TOL and e["cn"] <= CN_TOL, e


@pytest.mark.parametrize("name", list(dc.CASES))
def test_end_to_end_automatic_search(name, observed):
    got = _cached(name)
    ora = dc.oracle(name)
    c = dc.CASES[name]
    assert np.array_equal(got["center"], ora["center"]), (got["center"], ora["center"])
    K = ora["center"].shape[0]
    assert K >= 2 and got["A"].shape == ora["A"].shape and got["C"].shape == (K, c["T"])
    assert np.array_equal(got["ids"], np.arange(1, K + 1))
    e = dict(A=_maxrel(got["A"], ora["A"]), C=_maxrel(got["C"], ora["C"]), C_raw=_maxrel(got["C_raw"], ora["C_raw"]))
    if c.get("deconv"):
        S_o = np.array(ora["S"])
        e["C_fro"] = max(rel(got["C"][k], ora["C"][k]) for k in range(K))
        e["C_raw_fro"] = max(rel(got["C_raw"][k], ora["C_raw"][k]) for k in range(K))
        e["S_fro"] = max(rel(got["S"][k], S_o[k]) for k in range(K))
        e["gamma"] = float(np.max(np.abs(np.asarray(got["kernel_pars"], dtype=np.float64) - np.asarray(ora["kernel_pars"], dtype=np.float64))))
    observed["ds_e2e_%s" % name] = e
    print("ds init e2e %s: K %d  %s" % (name, K, {k: "%.3e" % v for k, v in e.items()}))
    if c["ssub"] != 1:
        assert (got["A"] < 0).any()                                        # the negative lobes of the bicubic kernel are kept
    else:
        assert np.array_equal(got["A"] != 0, ora["A"] != 0)
    if c.get("deconv"):
        assert e["A"] <= A_TOL
        assert e["C_fro"] <= DECONV_TOL and e["C_raw_fro"] <= DECONV_TOL and e["S_fro"] <= DECONV_TOL and e["gamma"] <= GAMMA_TOL, e
    else:
        assert e["A"] <= A_TOL and e["C"] <= C_TOL and e["C_raw"] <= C_TOL, e
        assert not got["S"].any()
    # the images returned are the seed images of the same object, bit for bit, where no trend is removed (nk > 1: initComponents_parallel detrends the full
    # series before the down-sampling, correlation_pnr_parallel the short one after it, as in the reference)
    if c.get("nk", 1) == 1:
        imgs = _cached_images(name)[0]
        assert np.array_equal(got["Cn"], imgs[0]) and np.array_equal(got["PNR"], imgs[1])


def test_two_runs_and_two_lanes_are_bit_identical():
    a, b, l2 = _cached("P"), _run("P"), _run("P", lanes=2)
    for other in (b, l2):
        assert np.array_equal(a["center"], other["center"]) and np.array_equal(a["A"], other["A"]) and np.array_equal(a["C"], other["C"])
        assert np.array_equal(a["Cn"], other["Cn"]) and np.array_equal(a["PNR"], other["PNR"])
    i1, i2 = _cached_images("S")
    assert np.array_equal(i1[0], i2[0]) and np.array_equal(i1[1], i2[1])
    il = _images("P", lanes=2)[0]
    assert np.array_equal(il[0], _cached_images("P")[0][0]) and np.array_equal(il[1], _cached_images("P")[0][1])


def test_refusals():
    from cnmf_e_amd import synth
    from cnmf_e_amd._lib import CnmfeError
    from cnmf_e_amd.engine import Engine
    from cnmf_e_amd.sources2d import Options, PatchedVideo, Sources2D, seed_psf
    d1, d2, T = 24, 20, 160
    f = synth.make_factors(d1, d2, T, 2, 5, gSig=1.5, gSiz=5, min_sep=4)
    Y = synth.make_video(f, np.float32)
    eng = Engine(0)
    try:
        video = PatchedVideo(d1, d2, T, [d1, d2], 3, eng)
        video.upload_from_full(Y)
        psf = seed_psf(1.5, 5, True)
        for call in (eng.seed_images_ds, eng.peel_open_ds):
            with pytest.raises(CnmfeError, match="error -5"):
                call(0, 1, 3, psf)                                         # Ts = 53 < 64
            with pytest.raises(CnmfeError, match="error -1"):
                call(0, 9, 1, psf)
            with pytest.raises(CnmfeError, match="error -1"):
                call(0, 0, 1, psf)
            with pytest.raises(CnmfeError, match="error -1"):
                call(0, 2, 0, psf)
        eng.patch_derive(0, 1, 2, "nearest")
        for call in (eng.seed_images_ds, eng.peel_open_ds):
            with pytest.raises(CnmfeError, match="error -5"):
                call(1, 2, 1, psf)                                         # a derived patch
        eng.peel_open_ds(0, 2, 2, psf)                                     # ... and no refused call left a session behind
        with pytest.raises(CnmfeError, match="error -4"):
            eng.peel_open_ds(0, 2, 2, psf)
        with pytest.raises(CnmfeError, match="error -1"):
            eng.peel_extract(0, 12, 5, 3)                                  # outside the 12 x 10 grid of the session
        corr, ai, ci, st = eng.peel_extract(0, 6, 5, 3)
        assert ci.shape == (80,) and corr.shape == (7, 7)
        eng.peel_close(0)
        s = Sources2D(video, Options(ring_radius=3, gSig=1.5, gSiz=5, ssub=2), f.A_init, f.C_init, f.sn)
        s.initComponents_parallel()
        with pytest.raises(NotImplementedError):
            s.initComponents_residual_parallel()                           # the second pass keeps its refusal
        s.options = Options(ring_radius=3, gSig=1.5, gSiz=5, ssub=2, tsub=2)
        with pytest.raises(NotImplementedError, match="constructed"):
            s.initComponents_parallel()                                    # the factors are declared at construction
        s.options = Options(ring_radius=3, gSig=1.5, gSiz=5, ssub=9)
        with pytest.raises(ValueError, match="9"):
            s.correlation_pnr_parallel()
        s = Sources2D(video, Options(ring_radius=3, gSig=1.5, gSiz=5, tsub=3), f.A_init, f.C_init, f.sn)
        with pytest.raises(ValueError, match="53"):
            s.initComponents_parallel()
    finally:
        eng.close()
