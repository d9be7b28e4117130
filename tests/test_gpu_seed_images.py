"""Seed images on the device: Sources2D.correlation_pnr_parallel (cnmfe_seed_images: k_seed_filter, k_seed_stats, k_seed_corr in csrc/seed.hpp) against the
float64 oracle tests/seed_oracle.py on the same seeded fp32 videos.

What is compared.  PNR on EVERY pixel, as a relative error.  Cn on every ROBUST pixel, as an absolute error: the threshold HY < 3 Sn
(correlation_image_endoscope.m:93) is a step, and a sample within the engine's rounding of it may fall on either side.  A pixel is FRAGILE when the oracle's
margin min_t |HY(t) - 3 Sn| / Sn is below delta = 1e-4 -- 3 x the engine's own GetSn bound of 2e-5 (test_estimate_noise_parity) plus the fp32 filter's rounding;
a pixel is left out of the Cn comparison when it or one of its 8 neighbours inside the block is fragile.  At most 10 % of a case may be left out (the oracle
alone gives 1.0 % (A), 0.5 % (E), 4.4 % (C), 1.8 % (D), 7.3 % (B), 1.9 % (F), 3.5 % (G)); the left-out pixels must still be finite and in [-1, 1].

Bounds: the rule of tests/test_gpu_parity.py -- 10 x the error observed on the MI355X, rounded up to one digit, never above the 1e-4 SURVEY 8(c) asks of fp32
quantities.  Observed on the MI355X (recorded per case through the `observed` fixture), PNR relative / Cn absolute on the robust pixels
(the same over all pixels: no threshold decision differed):
    A 9.8e-7 / 1.0e-7   E 1.1e-6 / 1.1e-7   C 1.7e-6 / 1.0e-7   D 1.8e-6 / 1.2e-7   B 2.6e-6 / 8.9e-8   F 6.6e-7 / 5.1e-8   G 5.4e-7 / 1.1e-7
The worst case sets each bound: PNR 2.6e-6 -> 3e-5, Cn 1.2e-7 -> 2e-6."""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import seed_oracle as so
from cnmf_e_amd import synth

pytestmark = pytest.mark.gpu

PNR_TOL = 3e-5        # relative, every pixel: 10 x 2.6e-6 (case B), rounded up
CN_TOL = 2e-6         # absolute, robust pixels: 10 x 1.2e-7 (case D), rounded up
MAX_LEFT_OUT = 0.10

#        d1, d2, T, K, seed, gSig, gSiz, patch dims, ring radius, options of the call
CASES = {
    "A": dict(dims=(44, 40), T=403, K=6, seed=29, gSig=1.5, gSiz=7, pdims=[22, 20], r=5),                          # 4 blocks with halo, odd T, T % 4 = 3
    "E": dict(dims=(44, 40), T=403, K=6, seed=29, gSig=1.5, gSiz=7, pdims=None, r=5, frame_range=(1, 250)),        # nframes % 4 = 2, even median
    "C": dict(dims=(40, 36), T=600, K=6, seed=3, gSig=2.0, gSiz=9, pdims=None, r=8),                               # replicate border at the image edge
    "D": dict(dims=(40, 36), T=600, K=6, seed=3, gSig=2.0, gSiz=9, pdims=None, r=8, nk=3),                         # detrend
    "B": dict(dims=(40, 36), T=600, K=6, seed=3, gSig=3.0, gSiz=13, pdims=None, r=8),                              # 113 taps, reach 6
    "F": dict(dims=(40, 36), T=600, K=6, seed=3, gSig=2.0, gSiz=9, pdims=None, r=8, center_psf=False),             # plain Gaussian
    "G": dict(dims=(40, 36), T=600, K=6, seed=3, gSig=2.0, gSiz=8, pdims=None, r=8, center_psf=False, synth_gSiz=9),   # round(gSiz) = 8: an even kernel, padded
}
_inputs, _oracle, _engine = {}, {}, {}


def _input(name):
    if name not in _inputs:
        c = CASES[name]
        f = synth.make_factors(c["dims"][0], c["dims"][1], c["T"], c["K"], c["seed"], gSig=c["gSig"], gSiz=int(c.get("synth_gSiz", c["gSiz"])))
        Y = synth.make_video(f, np.float32)
        Y.setflags(write=False)
        _inputs[name] = (f, Y)
    return _inputs[name]


def _run_engine(name, lanes=1, calls=1):
    """correlation_pnr_parallel of case `name` on a fresh engine: [(Cn, PNR)] * calls"""
    from cnmf_e_amd.engine import Engine
    from cnmf_e_amd.sources2d import PatchedVideo, Sources2D, Options
    c = CASES[name]
    f, Y = _input(name)
    d1, d2 = c["dims"]
    eng = Engine(0)
    try:
        if lanes != 1:
            eng.set_option("lanes", lanes)
        video = PatchedVideo(d1, d2, c["T"], c["pdims"] or [d1, d2], c["r"], eng)
        video.upload_from_full(Y)
        s = Sources2D(video, Options(ring_radius=c["r"], gSig=c["gSig"], gSiz=c["gSiz"], center_psf=c.get("center_psf", True), nk=c.get("nk", 1)),
                      f.A_init, f.C_init, f.sn)
        return [s.correlation_pnr_parallel(c.get("frame_range")) for _ in range(calls)]
    finally:
        eng.close()


def _engine_images(name):
    if name not in _engine:
        _engine[name] = _run_engine(name, calls=2)
    return _engine[name]


class _Geometry:
    def create_patch(self, *a):
        pass


def _oracle_images(name):
    if name not in _oracle:
        from cnmf_e_amd.sources2d import PatchedVideo
        c = CASES[name]
        _, Y = _input(name)
        d1, d2 = c["dims"]
        geo = PatchedVideo(d1, d2, c["T"], c["pdims"] or [d1, d2], c["r"], _Geometry())
        fr = c.get("frame_range")
        res = so.seed_images_fov(Y, geo, c["gSig"], c["gSiz"], c.get("center_psf", True), c.get("nk", 1), 3.0, None if fr is None else fr[1])
        for a in res:
            a.setflags(write=False)
        _oracle[name] = res
    return _oracle[name]


@pytest.mark.parametrize("name", list(CASES))
def test_seed_images_parity(name, observed):
    Cn, PNR = _engine_images(name)[0]
    Cn_o, PNR_o, robust = _oracle_images(name)
    d1, d2 = CASES[name]["dims"]
    assert Cn.shape == (d1, d2) and PNR.shape == (d1, d2) and Cn.dtype == np.float64 and PNR.dtype == np.float64
    assert np.all(np.isfinite(Cn)) and np.all(np.isfinite(PNR))
    e_pnr = float(np.max(np.abs(PNR - PNR_o) / np.abs(PNR_o)))
    e_cn = float(np.max(np.abs(Cn - Cn_o)[robust]))
    left = float((~robust).mean())
    e_cn_all = float(np.max(np.abs(Cn - Cn_o)))
    observed["seed_images_%s" % name] = dict(pnr_rel=e_pnr, cn_abs_robust=e_cn, cn_abs_all=e_cn_all, left_out=left)
    print("seed images %s: PNR rel %.3e  Cn abs (robust) %.3e  Cn abs (all pixels) %.3e  left out %.2f %%" % (name, e_pnr, e_cn, e_cn_all, 100 * left))
    assert left <= MAX_LEFT_OUT, left
    assert Cn.min() >= -1.0 and Cn.max() <= 1.0, (Cn.min(), Cn.max())
    assert e_pnr <= PNR_TOL, e_pnr
    assert e_cn <= CN_TOL, e_cn


def test_two_calls_return_equal_images():
    for name in ("A", "D"):
        (Cn1, PNR1), (Cn2, PNR2) = _engine_images(name)
        assert np.array_equal(Cn1, Cn2) and np.array_equal(PNR1, PNR2), name


def test_four_blocks_show_no_seam():
    """Case A's images are the oracle's per-block images merged the same way (test_seed_images_parity[A]).  Here: against ONE block over the whole FOV.  The
    7 x 7 filter reaches 3 pixels and the correlation one more; the halo is at least ring radius = 5 wide, so every patch pixel and its 8 neighbours see the
    whole FOV's filtered traces: the four-block images equal the whole-FOV ones on the rows and columns next to the cut lines as well as they do anywhere."""
    from cnmf_e_amd.sources2d import PatchedVideo
    c = CASES["A"]
    _, Y = _input("A")
    d1, d2 = c["dims"]
    Cn, PNR = _engine_images("A")[0]
    whole = PatchedVideo(d1, d2, c["T"], [d1, d2], c["r"], _Geometry())
    Cn_w, PNR_w, robust_w = so.seed_images_fov(Y, whole, c["gSig"], c["gSiz"], True, 1, 3.0)
    ok = _oracle_images("A")[2] & robust_w
    geo = PatchedVideo(d1, d2, c["T"], c["pdims"], c["r"], _Geometry())
    cut_r, cut_c = int(geo.patch_pos[(1, 0)][0]) - 1, int(geo.patch_pos[(0, 1)][2]) - 1      # 0-based first row / column of the second patch row / column
    seam = np.zeros((d1, d2), dtype=bool)
    seam[cut_r - 1:cut_r + 1, :] = True; seam[:, cut_c - 1:cut_c + 1] = True
    assert (seam & ok).sum() > 100
    assert np.max((np.abs(PNR - PNR_w) / np.abs(PNR_w))[seam]) <= PNR_TOL
    assert np.max(np.abs(Cn - Cn_w)[seam & ok]) <= CN_TOL
    assert np.max(np.abs(PNR - PNR_w) / np.abs(PNR_w)) <= PNR_TOL and np.max(np.abs(Cn - Cn_w)[ok]) <= CN_TOL


def test_two_lanes_give_the_same_images():
    ref = _engine_images("A")[0]
    got = _run_engine("A", lanes=2)[0]
    assert np.array_equal(got[0], ref[0]) and np.array_equal(got[1], ref[1])


def _iteration(with_seed):
    from cnmf_e_amd.engine import Engine
    from cnmf_e_amd.sources2d import PatchedVideo, Sources2D, Options
    c = CASES["A"]
    f, Y = _input("A")
    d1, d2 = c["dims"]
    eng = Engine(0)
    try:
        video = PatchedVideo(d1, d2, c["T"], c["pdims"], c["r"], eng)
        video.upload_from_full(Y)
        s = Sources2D(video, Options(ring_radius=c["r"], maxIter=3, gSig=c["gSig"], gSiz=c["gSiz"]), f.A_init, f.C_init, f.sn)
        if with_seed:
            s.correlation_pnr_parallel()
        s.update_background_parallel()
        W = [s.get_W(idx).data.copy() for idx in video.owned]
        s.update_spatial_parallel()
        A = s.A.toarray()
        s.update_temporal_parallel()
        return W, A, np.asarray(s.C, dtype=np.float32).copy()
    finally:
        eng.close()


def test_an_iteration_after_the_seed_images_is_unchanged():
    W0, A0, C0 = _iteration(False)
    W1, A1, C1 = _iteration(True)
    assert all(np.array_equal(a, b) for a, b in zip(W0, W1))
    assert np.array_equal(A0, A1) and np.array_equal(C0, C1)
    assert np.all(np.isfinite(C0)) and A0.any()


def test_the_hot_set_contains_every_true_centre():
    f, _ = _input("C")
    Cn, PNR = _engine_images("C")[0]
    hot = ((Cn > 0.8) & (PNR > 8)).reshape(-1, order="F")
    for k in range(f.K):
        ctr = int(np.argmax(f.A_true[:, k].toarray().ravel()))
        assert hot[ctr], (k, ctr, Cn.reshape(-1, order="F")[ctr], PNR.reshape(-1, order="F")[ctr])


def test_outside_the_envelope_is_unsupported():
    from cnmf_e_amd.engine import Engine
    from cnmf_e_amd._lib import CnmfeError
    from cnmf_e_amd.sources2d import PatchedVideo, seed_psf
    d1, d2, T = 24, 20, 80
    eng = Engine(0)
    try:
        video = PatchedVideo(d1, d2, T, [d1, d2], 3, eng)
        video.upload_from_full(np.random.default_rng(0).standard_normal((T, d1 * d2)).astype(np.float32))
        psf = seed_psf(1.5, 7, True)
        for kw in (dict(nframes=40), dict(nframes=T + 1), dict(frame0=4, nframes=64)):
            with pytest.raises(CnmfeError, match="error -5"):
                eng.seed_images(0, psf, **kw)
        with pytest.raises(CnmfeError, match="error -5"):
            eng.seed_images(0, np.ones((4, 4)) / 16)                      # an even kernel: the caller pads it (seed_psf)
        with pytest.raises(CnmfeError, match="error -5"):
            eng.seed_images(0, np.ones((27, 27)) / 729)
        with pytest.raises(CnmfeError, match="error -5"):
            eng.seed_images(0, psf, Q=np.linalg.qr(np.random.default_rng(1).standard_normal((T, 17)))[0])
        eng.patch_derive(0, 1, 2, "nearest")
        with pytest.raises(CnmfeError, match="error -5"):
            eng.seed_images(1, psf)
        Cn, PNR = eng.seed_images(0, psf)                                 # ... and the refused calls left the patch usable; no filter is a valid request
        Cn0, PNR0 = eng.seed_images(0, None, nframes=64)
        assert np.all(np.isfinite(Cn)) and np.all(np.isfinite(PNR)) and np.all(np.isfinite(Cn0)) and np.all(PNR0 > 0)
    finally:
        eng.close()
