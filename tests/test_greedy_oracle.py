"""CPU tests of the greedy initialisation's host functions (cnmf_e_amd/hostops.py) and of the float64 oracle tests/greedy_oracle.py, and the FIXTURE CHECK
that entitles tests/test_gpu_init.py to demand identical discrete decisions: for every case the oracle's decision margins clear the fixture bounds of
tests/greedy_cases.py (10 x the bounds tests/test_gpu_seed_images.py asserts for Cn and PNR, 1e-4 for the correlation sets, 1e-4 relative for the rest)."""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import greedy_cases as gc
import greedy_oracle as go
import cnmfe_oracle as orc
from cnmf_e_amd import hostops


def test_fit_gauss1_recovers_a_sampled_gaussian():
    x = np.linspace(-3.0, 9.0, 121)
    for fit in (hostops.fit_gauss1, go.fit_gauss1):
        mu, sig, A = fit(x, 7.0 * np.exp(-(x - 2.5) ** 2 / (2 * 1.3 ** 2)), 0.3, 3)
        assert abs(mu - 2.5) < 1e-9 and abs(sig - 1.3) < 1e-9 and abs(A - 7.0) < 1e-8
    mu, sig, A = hostops.fit_gauss1(x, 4.0 * np.exp(-x ** 2 / (2 * 0.8 ** 2)), 0.3, 3, True)
    assert mu == 0.0 and abs(sig - 0.8) < 1e-9 and abs(A - 4.0) < 1e-8


def _trace(seed, T=6000, b=3.0, sn=0.7):
    rng = np.random.default_rng(seed)
    s = (rng.random(T) < 0.002) * rng.uniform(5, 15, T)
    c = np.zeros(T)
    for t in range(1, T):
        c[t] = 0.8 * c[t - 1] + s[t]
    return b + sn * rng.standard_normal(T) + c


def test_estimate_baseline_noise_on_a_transient_trace():
    """baseline + white noise + sparse positive transients: the fit to the histogram's mode returns both within the sampling error of the 6000 samples (the
    transients occupy about 3 % of the frames and leave the mode alone; 0.1 sn is 8 standard errors of a mean of 6000 samples, the allowance for a fit that
    reads the mode off histogram counts instead of averaging)"""
    for seed in range(3):
        b, sn = hostops.estimate_baseline_noise(_trace(seed))
        assert abs(b - 3.0) < 0.1 * 0.7 and abs(sn - 0.7) < 0.1 * 0.7, (seed, b, sn)


def test_host_baseline_functions_equal_the_oracles():
    for seed in range(4):
        y = _trace(10 + seed, T=1500)
        b, sn = hostops.estimate_baseline_noise(y)
        bo, sno = go.estimate_baseline_noise(y)
        assert abs(b - bo) <= 1e-9 * abs(bo) and abs(sn - sno) <= 1e-9 * sno
        q = np.arange(11) / 10.0
        assert np.allclose(hostops.matlab_quantile(y, q), [orc.matlab_quantile(y, p) for p in q], rtol=0, atol=1e-12)
        bins = np.linspace(y.min(), y.max(), 37)
        assert np.array_equal(hostops.hist_centres(y, bins), go.hist_centres(y, bins))
        assert hostops.hist_centres(y, bins).sum() == y.size
        r, br = hostops.remove_baseline(y, sno)
        ro, bro = go.remove_baseline(y, sno)
        assert br == bro and np.array_equal(r, ro)
    assert hostops.estimate_baseline_noise(np.full(50, 2.0)) == (2.0, 0.0)


@pytest.mark.parametrize("n", [3, 4, 5])
def test_window_maximum_equals_brute_force(n):
    rng = np.random.default_rng(n)
    v = rng.random((13, 11)) * (rng.random((13, 11)) > 0.4)
    got = hostops.ordfilt2_max(v, n)
    assert np.array_equal(got, go.window_max_brute(v, n))
    # an even window is NOT centred: it reaches one pixel further down / right (origin floor((n + 1) / 2))
    if n == 4:
        e = np.zeros((9, 9)); e[4, 4] = 1.0
        assert np.array_equal(np.argwhere(hostops.ordfilt2_max(e, 4) == 1), [[r, c] for r in range(2, 6) for c in range(2, 6)])


def test_host_connectivity_equals_the_oracles():
    rng = np.random.default_rng(5)
    for k in range(6):
        y, x = np.mgrid[:19, :17]
        img = np.exp(-((y - 8) ** 2 + (x - 7) ** 2) / 18.0) + 0.6 * np.exp(-((y - 2 - k) ** 2 + (x - 14) ** 2) / 6.0)
        img = img * (rng.random(img.shape) > 0.1)
        assert np.array_equal(hostops.connectivity_constraint(img), orc.connectivity_constraint(img))
    assert np.array_equal(hostops.circular_constraints(img), orc.circular_constraints(img))


def test_host_filter_equals_the_oracles():
    import seed_oracle as so
    rng = np.random.default_rng(2)
    img = rng.random((15, 12))
    for psf in (so.make_psf(2.0, 9, True), so.make_psf(2.0, 8, False)):
        assert np.allclose(hostops.imfilter_replicate(img, psf), so.imfilter_replicate(img[:, :, None], psf)[:, :, 0], rtol=0, atol=1e-14)


class _OracleSession:
    """the oracle's own arithmetic behind the host loop's session interface: the host loop (hostops.greedy_roi_block) must then retrace the oracle's run"""
    def __init__(self, Yb, nr, nc, gSig, gSiz, nk):
        import oasis_oracle as oo
        import seed_oracle as so
        Y = np.array(Yb, dtype=np.float64)
        if nk > 1:
            Y = so.detrend_spline(Y, nk)
        self.psf = so.make_psf(gSig, gSiz, True)
        T = Y.shape[1]
        HY = so.imfilter_replicate(Y.reshape(nr, nc, T, order="F"), self.psf).reshape(nr * nc, T, order="F")
        self.HY = HY - np.median(HY, axis=1, keepdims=True)
        self.Sn = np.array([oo.GetSn(row) for row in self.HY])
        self.Y, self.nr, self.nc, self.gSiz, self.so, self.oo = Y, nr, nc, gSiz, so, oo
        self.PNR = (self.HY.max(axis=1) / self.Sn).reshape(nr, nc, order="F")
        self.Cn = so.correlation_image(np.where(self.HY < 3 * self.Sn[:, None], 0.0, self.HY), nr, nc)

    def extract(self, r, c):
        r0, r1, c0, c1 = go._box(self.nr, self.nc, r, c, self.gSiz)
        ind = go._box_pixels(self.nr, r0, r1, c0, c1)
        y0 = self.HY[c * self.nr + r]
        corr = go.pearson_rows(y0, self.HY[ind])
        hi, lo = corr > 0.9, corr < 0.3
        ci = self.HY[ind][hi].mean(axis=0)
        X = np.stack([np.ones(ci.size), np.median(self.Y[ind][lo], axis=0), ci], axis=1)
        ai = np.maximum(0.0, np.linalg.lstsq(X, self.Y[ind].T, rcond=None)[0][2])
        dy = np.diff(y0)
        st = dict(max_diff=dy.max(), std_diff=dy.std(ddof=1), norm_ci=np.linalg.norm(ci), sn_ci=self.oo.GetSn(ci), n_hi=int(hi.sum()), n_lo=int(lo.sum()))
        sh = (r1 - r0, c1 - c0)
        return corr.reshape(sh, order="F"), ai.reshape(sh, order="F"), ci, st

    def apply(self, r, c, ai, Hai, ci, sig, min_pnr, min_corr):
        r0, r1, c0, c1 = go._box(self.nr, self.nc, r, c, self.gSiz)
        s0, s1, t0, t1 = go._box(self.nr, self.nc, r, c, 2 * self.gSiz)
        ind, ind2 = go._box_pixels(self.nr, r0, r1, c0, c1), go._box_pixels(self.nr, s0, s1, t0, t1)
        self.Y[ind] -= np.outer(ai.reshape(-1, order="F"), ci)
        self.HY[ind2] -= np.outer(Hai.reshape(-1, order="F"), ci)
        H2, S2 = self.HY[ind2], self.Sn[ind2]
        pnr = H2.max(axis=1) / S2
        pnr[np.isnan(pnr) | (pnr < min_pnr)] = 0
        cn = self.so.correlation_image(np.where(H2 < sig * S2[:, None], 0.0, H2), s1 - s0, t1 - t0)
        cn[np.isnan(cn) | (cn < min_corr)] = 0
        return pnr.reshape(s1 - s0, t1 - t0, order="F"), cn


def test_host_loop_retraces_the_oracle():
    """hostops.greedy_roi_block over the oracle's arithmetic finds the oracle's neurons: same centres in the same order, equal footprints and traces (case B)"""
    c = gc.CASES["B"]
    _, Y = gc.inputs("B")
    nr, nc = c["dims"]
    o = gc.oracle("B")["blocks"][(0, 0)]
    sess = _OracleSession(Y.T, nr, nc, c["gSig"], c["gSiz"], 1)
    res = hostops.greedy_roi_block(sess, sess.Cn, sess.PNR, c["gSiz"], sess.psf, 0.3, 10.0, 5.0, [3, 3, 3, 3])
    assert np.array_equal(res["center"], o["center"]) and len(res["A"]) >= 1
    for k in range(len(res["A"])):
        assert res["A"][k][0] == o["A"][k][0]
        assert np.allclose(res["A"][k][1], o["A"][k][1], rtol=1e-9, atol=1e-12) and np.allclose(res["C"][k], o["C"][k], rtol=1e-9, atol=1e-12)


def _margins(name, forced):
    return gc.oracle(name, forced)["margins"]


@pytest.mark.parametrize("forced", [False, True], ids=["auto", "forced"])
@pytest.mark.parametrize("name", list(gc.CASES))
def test_fixture_margins(name, forced):
    """FIXTURE CHECK: every comparison the oracle's run makes is decided by at least the fixture bound, for the automatic search and for the forced-seed run
    of test 1.  A case that fails here needs another synthetic seed, not another bound."""
    res = gc.oracle(name, forced)
    mg = res["margins"]
    print(name, "forced" if forced else "auto", "K", res["center"].shape[0], {k: "%.2e" % v for k, v in sorted(mg.items())})
    assert res["center"].shape[0] >= 1
    for key in ("corr", "cn", "pnr", "diff", "hy"):
        assert key in mg, key
    for key, val in mg.items():
        assert val >= gc.MARGIN_MIN.get(key, gc.MARGIN_DEFAULT), (name, key, val)
