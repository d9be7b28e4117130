"""The seed images' float64 oracle (tests/seed_oracle.py) against an independent statement of what it computes, and the host helpers of
Sources2D.correlation_pnr_parallel: the filter (seed_psf), the detrend basis (bspline_basis), the options it refuses.  No GPU."""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import seed_oracle as so
from cnmf_e_amd import synth
from cnmf_e_amd.sources2d import Options, PatchedVideo, Sources2D, bspline_basis, seed_psf


def test_oracle_cn_is_the_mean_pearson_correlation_with_the_8_neighbours():
    d1, d2, T = 10, 9, 300
    f = synth.make_factors(d1, d2, T, 1, 17, gSig=1.5, gSiz=5)
    Y = synth.make_video(f, np.float32).astype(np.float64).T              # d x T
    # sig = 1: every thresholded trace keeps samples, so every Pearson coefficient is defined (at 3 Sn most noise-only traces of 300 frames are all zero)
    HY, _, _ = so.filtered_traces(Y, d1, d2, 1.5, 5, True, 1, sig=1.0)
    assert np.all(HY.std(axis=1) > 0)
    Cn = so.correlation_image(HY, d1, d2)
    R = np.corrcoef(HY)
    ref = np.zeros((d1, d2))
    for r in range(d1):
        for c in range(d2):
            nb = [(r + a, c + b) for a in (-1, 0, 1) for b in (-1, 0, 1) if (a or b) and 0 <= r + a < d1 and 0 <= c + b < d2]
            ref[r, c] = np.mean([R[c * d1 + r, cc * d1 + rr] for rr, cc in nb])
    assert np.abs(Cn - ref).max() <= 1e-12, np.abs(Cn - ref).max()
    # ... and the whole-block entry point is those two steps
    Cn2, PNR, margin = so.seed_images(Y, d1, d2, 1.5, 5, True, 1, sig=1.0)
    assert np.array_equal(Cn2, Cn) and PNR.shape == (d1, d2) and np.all(margin >= 0)


@pytest.mark.parametrize("gSig,n,support", [(3.0, 13, 113), (2.0, 9, 49), (1.5, 7, 29)])
def test_seed_psf_centred_support_and_zero_sum(gSig, n, support):
    psf = seed_psf(gSig, 4 * gSig + 1, True)
    assert psf.shape == (n, n) and int((psf != 0).sum()) == support
    assert abs(psf.sum()) <= 1e-15
    assert np.array_equal(psf, psf.T) and np.array_equal(psf, psf[::-1, ::-1])
    assert np.array_equal(psf, so.make_psf(gSig, 4 * gSig + 1, True))


def test_seed_psf_plain_gaussian_and_the_padding_of_an_even_kernel():
    assert seed_psf(0, 9, True) is None and seed_psf(-1.0, 9, False) is None
    odd = seed_psf(2.0, 9, False)
    assert odd.shape == (9, 9) and abs(odd.sum() - 1) <= 1e-15 and np.all(odd > 0)
    assert seed_psf(2.0, 8.5, False).shape == (9, 9)                      # round(8.5) = 9: MATLAB rounds halves away from zero
    even = seed_psf(2.0, 8, False)
    raw = so.make_psf(2.0, 8, False)
    assert raw.shape == (8, 8) and even.shape == (9, 9)
    assert np.all(even[0, :] == 0) and np.all(even[:, 0] == 0) and np.array_equal(even[1:, 1:], raw)
    # the padded odd kernel filters about its centre exactly as imfilter filters the even one about floor((n + 1) / 2)
    Y3 = np.random.default_rng(0).standard_normal((12, 11, 3))
    assert np.array_equal(so.imfilter_replicate(Y3, even), so.imfilter_replicate(Y3, raw))
    from scipy.ndimage import correlate
    ref = np.stack([correlate(Y3[:, :, t], even, mode="nearest") for t in range(3)], axis=2)
    assert np.abs(so.imfilter_replicate(Y3, even) - ref).max() <= 1e-14


@pytest.mark.parametrize("T,nk", [(300, 3), (403, 2), (250, 5), (64, 3)])
def test_bspline_basis_equals_scipy_design_matrix(T, nk):
    from scipy.interpolate import BSpline
    X = bspline_basis(T, nk)
    br = np.linspace(1.0, float(T), nk)
    ref = BSpline.design_matrix(np.arange(1, T + 1, dtype=np.float64), np.r_[[br[0]] * 3, br, [br[-1]] * 3], 3).toarray()
    assert X.shape == (T, nk + 2)
    assert np.abs(X - ref).max() <= 1e-12
    assert np.abs(X.sum(axis=1) - 1).max() <= 1e-12
    assert np.linalg.matrix_rank(X) == nk + 2


def _sources(**opt):
    from fake_engine import FakeEngine
    d1, d2, T, r = 24, 20, 80, 3
    f = synth.make_factors(d1, d2, T, 2, 5, gSig=1.5, gSiz=5, min_sep=4)
    v = PatchedVideo(d1, d2, T, [d1, d2], r, FakeEngine())
    v.upload_from_full(synth.make_video(f, np.float32))
    return Sources2D(v, Options(ring_radius=r, **opt), f.A_init, f.C_init, f.sn)


@pytest.mark.parametrize("opt,fr", [(dict(ssub=2), None), (dict(tsub=2), None), (dict(nk=3, detrend_method="local_min"), None),
                                    (dict(), (5, 80)), (dict(), (2, 70))], ids=["ssub", "tsub", "local_min", "range_5_80", "range_2_70"])
def test_correlation_pnr_parallel_refuses_what_is_not_built(opt, fr):
    s = _sources(**opt)
    with pytest.raises(NotImplementedError):
        s.correlation_pnr_parallel(fr)


def test_correlation_pnr_parallel_hands_the_engine_the_filter_the_basis_and_the_clipped_range():
    s = _sources(gSig=1.5, gSiz=5, nk=3)
    seen = []

    def seed_images(pid, psf, nframes=None, Q=None, sig=3.0):
        seen.append((pid, psf, nframes, Q, sig))
        d_b = s.video.block_pix[(0, 0)].size
        return np.arange(d_b, dtype=np.float32), -np.arange(d_b, dtype=np.float32)
    s.engine.seed_images = seed_images
    Cn, PNR = s.correlation_pnr_parallel((0, 500))                        # clipped to [1, T] (correlation_pnr_parallel.m:43-44)
    (pid, psf, n, Q, sig), = seen
    assert pid == 0 and n == 80 and sig == 3.0 and np.array_equal(psf, seed_psf(1.5, 5, True))
    assert Q.shape == (80, 5) and np.abs(Q.T @ Q - np.eye(5)).max() <= 1e-12
    X = bspline_basis(80, 3)
    assert np.abs(Q @ (Q.T @ X) - X).max() <= 1e-12                       # the same span
    assert Cn.dtype == np.float64 and Cn.shape == (24, 20) and PNR.shape == (24, 20)
    assert np.array_equal(Cn.reshape(-1, order="F"), np.arange(24 * 20)) and np.array_equal(PNR, -Cn)
    assert not hasattr(Options(), "no_such") and Options().nk == 1 and Options().gSig == 3.0 and Options().center_psf is True
