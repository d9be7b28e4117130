"""The float64 oracle of the down-sampled initialisation (tests/ds_oracle.py) against independent statements of the same definitions, the product's host
restatements (hostops.imresize_matrix) against it, the two-pass pre-detrend algebra the device uses, the Options checks, and the decision margins of the
fixtures of tests/ds_cases.py.  No GPU."""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import ds_cases as dc
import ds_oracle as dso
import seed_oracle as so
from cnmf_e_amd import hostops, synth
from cnmf_e_amd.sources2d import Options, PatchedVideo, Sources2D, bspline_basis


def _pil_resize(img, out_hw, resample):
    from PIL import Image
    im = Image.fromarray(np.asarray(img, dtype=np.float32), mode="F")
    return np.asarray(im.resize((out_hw[1], out_hw[0]), resample=resample), dtype=np.float64)


@pytest.mark.parametrize("ssub", [2, 3, 4])
def test_box_downsampling_of_a_divisible_size_is_the_block_mean(ssub):
    rng = np.random.default_rng(ssub)
    nr, nc, T = 6 * ssub, 5 * ssub, 7
    Y = rng.standard_normal((nr, nc, T))
    got = dso.ds_data(Y, ssub, 1)
    ref = Y.reshape(6, ssub, 5, ssub, T).mean(axis=(1, 3))
    assert got.shape == ref.shape and np.abs(got - ref).max() <= 1e-14


def test_temporal_step_is_the_mean_of_tsub_frames_and_drops_the_rest():
    rng = np.random.default_rng(1)
    Y = rng.standard_normal((4, 3, 23))
    got = dso.ds_data(Y, 1, 5)
    assert got.shape == (4, 3, 4)
    for t in range(4):
        assert np.abs(got[:, :, t] - Y[:, :, 5 * t:5 * t + 5].mean(axis=2)).max() <= 1e-15


@pytest.mark.parametrize("tsub", [2, 3, 5])
def test_box_upsampling_of_whole_bins_is_repeat(tsub):
    rng = np.random.default_rng(tsub)
    X = rng.standard_normal((3, 17))
    assert np.array_equal(dso.up_time(X, 17 * tsub, "box"), np.repeat(X, tsub, axis=1))


def test_box_and_bicubic_agree_with_pillow_in_the_interior():
    """Pillow's BOX and BICUBIC resizes are the constructions the toolbox documents (centre-aligned samples, the kernel stretched by 1 / scale when shrinking,
    normalised weights); they differ in how the window is closed at the border (mirrored here, clipped there), so a rim is left out.  Pillow works in fp32."""
    from PIL import Image
    rng = np.random.default_rng(4)
    img = rng.standard_normal((48, 60)).cumsum(axis=0).cumsum(axis=1)
    for out in ((24, 30), (16, 20)):                                       # sizes the factor divides: Pillow's box support equals the half-open one
        got = dso.imresize(img, out, "box")
        ref = _pil_resize(img, out, Image.BOX)
        assert np.abs(got - ref).max() / np.abs(ref).max() <= 2e-6
    got = dso.imresize(img, (17, 23), "bicubic")
    ref = _pil_resize(img, (17, 23), Image.BICUBIC)
    assert np.abs(got - ref)[3:-3, 3:-3].max() / np.abs(ref).max() <= 2e-6
    small = rng.standard_normal((20, 24)).cumsum(axis=0)
    got = dso.imresize(small, (40, 47), "bicubic")
    ref = _pil_resize(small, (40, 47), Image.BICUBIC)
    assert np.abs(got - ref)[5:-5, 5:-5].max() / np.abs(ref).max() <= 2e-6


@pytest.mark.parametrize("n_in,n_out", [(45, 15), (37, 13), (44, 22), (33, 17), (26, 13), (40, 5), (13, 37), (15, 45), (201, 403), (150, 600), (200, 600), (7, 7)])
@pytest.mark.parametrize("method", ["box", "bicubic"])
def test_hostops_resize_matrices_equal_the_oracles(n_in, n_out, method):
    M, ref = hostops.imresize_matrix(n_in, n_out, method), dso.resize_weights(n_in, n_out, method)
    assert M.shape == (n_out, n_in) and np.abs(M - ref).max() <= 1e-14
    assert np.abs(M.sum(axis=1) - 1).max() <= 1e-14
    if n_in == n_out:
        assert np.array_equal(M, np.eye(n_in))


def test_a_size_ssub_does_not_divide_mirrors_at_the_border():
    """37 -> 13 columns: scale 13 / 37, windows of 37 / 13 = 2.85 pixels hold 2 or 3 of them, the last one reaches past the edge and is mirrored"""
    M = dso.resize_weights(37, 13, "box")
    cnt = (M > 0).sum(axis=1)
    assert set(cnt) <= {2, 3} and cnt.min() == 2 and cnt.max() == 3
    assert np.all((M > 0).sum(axis=0) >= 1)                                # every input pixel is used


def test_two_pass_predetrend_equals_detrend_then_downsample():
    """dsData(Y - (Y Q) Q') = dsData(Y) - mean_bin(Q) (box(Y) Q)': the algebra of k_ds_coef + k_ds_video, with an orthonormal basis of the splines' span"""
    rng = np.random.default_rng(9)
    nr, nc, T, ssub, tsub, nk = 11, 9, 203, 2, 4, 3
    Y = 100 + rng.standard_normal((nr * nc, T)).cumsum(axis=1)
    ref, d1s, d2s = dso.peel_video(Y, nr, nc, nk, ssub, tsub)
    Q = np.linalg.qr(bspline_basis(T, nk))[0]
    Yc = Y - Y.mean(axis=1, keepdims=True)                                 # the resident video is centred; the mean lies in the span
    Ys = dso.imresize(Yc.reshape(nr, nc, T, order="F"), (d1s, d2s), "box").reshape(d1s * d2s, T, order="F")
    G = Ys @ Q
    Ts = T // tsub
    bm = Q[:Ts * tsub].reshape(Ts, tsub, -1).mean(axis=1)
    got = Ys[:, :Ts * tsub].reshape(-1, Ts, tsub).mean(axis=2) - G @ bm.T
    assert np.abs(got - ref).max() <= 1e-12 * np.abs(Y).max()


def _sources(T=160, **opt):
    from fake_engine import FakeEngine
    d1, d2, r = 24, 20, 3
    f = synth.make_factors(d1, d2, T, 2, 5, gSig=1.5, gSiz=5, min_sep=4)
    v = PatchedVideo(d1, d2, T, [d1, d2], r, FakeEngine())
    v.upload_from_full(synth.make_video(f, np.float32))
    s = Sources2D(v, Options(ring_radius=r, **opt), f.A_init, f.C_init, f.sn)
    s.engine.supports_init_ds = True                                     # (the double stands for an engine with the down-sampled entry points)
    return s


@pytest.mark.parametrize("opt,msg", [(dict(ssub=9), "ssub.*9"), (dict(ssub=0), "ssub.*0"), (dict(ssub=1.5), "ssub.*1.5"), (dict(tsub=0), "tsub.*0"),
                                     (dict(tsub=3), r"floor\(160 / 3\) = 53")])
def test_options_are_validated_with_the_numbers_in_the_message(opt, msg):
    s = _sources(**opt)
    with pytest.raises(ValueError, match=msg):
        s.correlation_pnr_parallel()
    with pytest.raises(ValueError, match=msg):
        s.initComponents_parallel()


def test_factors_are_declared_at_construction_and_need_an_engine_that_builds_them():
    s = _sources(ssub=2)
    s.options = Options(ring_radius=3, ssub=2, tsub=2)                     # swapped in later with other factors
    with pytest.raises(NotImplementedError, match="constructed with ssub = 2, tsub = 1"):
        s.correlation_pnr_parallel()
    with pytest.raises(NotImplementedError, match="constructed"):
        s.initComponents_parallel()
    s = _sources(tsub=2)
    s.engine.supports_init_ds = False
    with pytest.raises(NotImplementedError, match="supports_init_ds"):
        s.correlation_pnr_parallel()


def test_the_second_pass_still_refuses():
    for opt in (dict(ssub=2), dict(tsub=2)):
        with pytest.raises(NotImplementedError):
            _sources(**opt).initComponents_residual_parallel()


def test_correlation_pnr_parallel_hands_the_engine_the_scaled_filter_and_the_short_basis():
    from cnmf_e_amd.sources2d import seed_psf
    s = _sources(T=160, gSig=3.0, gSiz=9, nk=3, ssub=2, tsub=2)
    seen = []

    def seed_images_ds(pid, ssub, tsub, psf, nframes=None, Q=None, sig=3.0):
        seen.append((pid, ssub, tsub, psf, nframes, Q, sig))
        return np.full(12 * 10, 0.5, dtype=np.float32), np.full(12 * 10, 7.0, dtype=np.float32)
    s.engine.seed_images_ds = seed_images_ds
    Cn, PNR = s.correlation_pnr_parallel()
    (pid, ssub, tsub, psf, n, Q, sig), = seen
    assert (pid, ssub, tsub, n, sig) == (0, 2, 2, 160, 3.0) and np.array_equal(psf, seed_psf(1.5, 5, True))
    assert Q.shape == (80, 5) and np.abs(Q.T @ Q - np.eye(5)).max() <= 1e-12
    assert Cn.shape == (24, 20) and np.abs(Cn - 0.5).max() <= 1e-12 and np.abs(PNR - 7.0).max() <= 1e-12      # a constant image is resized to itself


@pytest.mark.parametrize("forced", [False, True], ids=["auto", "forced"])
@pytest.mark.parametrize("name", list(dc.CASES))
def test_fixture_margins(name, forced):
    """FIXTURE CHECK: every comparison the oracle's run makes on the low-resolution video is decided by at least the fixture bound, for the automatic search
    and for the forced-seed run.  A case that fails here needs another synthetic seed, not another bound."""
    res = dc.oracle(name, forced)
    mg = res["margins"]
    print(name, "forced" if forced else "auto", "K", res["center"].shape[0], {k: "%.2e" % v for k, v in sorted(mg.items())})
    assert res["center"].shape[0] >= 2
    if forced:
        assert np.array_equal(res["center"], dc.oracle(name)["center"])
    for key in ("corr", "cn", "pnr", "diff", "hy"):
        assert key in mg, key
    for key, val in mg.items():
        assert val >= dc.MARGIN_MIN.get(key, dc.MARGIN_DEFAULT), (name, key, val)


@pytest.mark.parametrize("name", list(dc.CASES))
def test_fixture_seed_images_leave_out_at_most_a_tenth(name):
    robust = dc.oracle_images(name)[2]
    left = float((~robust).mean())
    print(name, "left out %.2f %%" % (100 * left))
    assert left <= 0.10


def test_center_rule_and_upsampled_shapes():
    """case Q: center = center * ssub - 1 on the block, footprints on the full grid with the negative lobes of the bicubic kernel kept"""
    res = dc.oracle("Q")
    blk = res["blocks"][(0, 0)]
    assert np.array_equal(blk["center"], blk["low"]["center"] * 3 - 1)
    d1, d2 = dc.CASES["Q"]["dims"]
    assert res["A"].shape[0] == d1 * d2 and res["C"].shape[1] == dc.CASES["Q"]["T"]
    assert (res["A"] < 0).any()
