"""k_deconv against the float64 oracle across its option branches, trace edges and pool sizes (tests/deconv_branch_cases.py; the rows are shown to reach
their branches and to be well-conditioned by tests/test_deconv_branch_cases.py, on the oracle alone).

Every case is one deconv_temporal call on the case's float32 values; the oracle runs on the same values cast to float64.  The bounds this path has elsewhere
(sn rtol 5e-6, gamma 2e-6 absolute, traces 5e-6 relative Frobenius) were all more than 10x above what these cases show on an MI355X, so each is set just
under 10x the largest value observed over all cases.  S, compared by spike count alone until now, must have the oracle's support sample
by sample and its values within S_TOL.

Observed maxima per family (sn relative, gamma absolute, C / C_raw / S relative Frobenius per row):
  options  sn 1.1e-7  gamma 3.3e-8  C 2.8e-7  C_raw 8.2e-8  S 1.7e-7        pools  sn 2.5e-7  gamma 2.9e-8  C 3.2e-8  C_raw 3.7e-8  S 4.3e-8
  ties     sn 9.1e-8  gamma 2.6e-8  C 3.9e-8  C_raw 5.5e-8  S 6.7e-8        white  sn 9.2e-8  gamma 2.9e-8  C 2.5e-8  C_raw 2.9e-8  S 0 (no spikes)
  period2  sn 7.0e-8  (give-up rows: exact)                                 hals   sn 9.5e-8  gamma 1.4e-7  C 7.9e-8  C_raw 9.3e-8  S 7.3e-8"""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu

import deconv_branch_cases as dbc
from parity_util import rel

SN_RTOL = 2.4e-6        # observed 2.5e-7 (pools, T = 193)
PARS_ATOL = 1.4e-6      # observed 1.4e-7 (hals, the row below gmax: update_g from a preset gamma)
C_TOL = 2.7e-6          # observed 2.8e-7 (options)
C_RAW_TOL = 9e-7        # observed 9.3e-8 (hals)
# s(t) = c(t) - g c(t - 1) is formed from two fp32-rounded values of c; measured for the first time here, it is no worse than C: observed 1.7e-7 (options),
# bound 10x that (the ceiling for traces, SURVEY.md 8(c), is 1e-4)
S_TOL = 1.7e-6


@pytest.fixture(scope="module")
def eng():
    from cnmf_e_amd.engine import Engine
    e = Engine(0)
    yield e
    e.close()


def _note(observed, family, **vals):
    rec = observed.setdefault("deconv_branches", {}).setdefault(family, {})
    for k, v in vals.items():
        rec[k] = max(rec.get(k, 0.0), float(v))


def _compare_row(name, k, tag, y32, got, ref, g_first):
    """one row of a case against the oracle; returns the observed figures (sn, pars, C, C_raw, S)"""
    Cg, Crawg, Sg, parsg, sng = got
    Cr, Crawr, Sr, parsr, snr = ref
    if tag == "nan":                                            # deconvTemporal.m:37-40
        assert not Cg.any() and not Sg.any() and not Crawg.any() and parsg == 0 and sng == 0, (name, k)
        return None
    d_sn = abs(sng / snr - 1)
    assert d_sn <= SN_RTOL, (name, k, sng, snr)                                     # observed 2.5e-7
    if tag == "giveup":                                         # deconvolveCa.m:84-89, deconvTemporal.m:53-55
        assert parsg == 0 and not Sg.any(), (name, k, parsg)
        assert np.array_equal(Cg, Crawg) and np.array_equal(Crawg, y32), (name, k)
        return dict(sn=d_sn)
    d_g = abs(float(parsg) - parsr)
    if tag == "restart":                                        # foopsi_oasisAR1.m:104-108: the re-estimate, not update_g's minimiser
        assert abs(float(parsg) - g_first) <= PARS_ATOL, (name, k, "no restart", float(parsg), g_first, parsr)
    if tag == "update_g":                                       # :82-90: update_g ran although g > gmax
        assert abs(float(parsg) - g_first) > 1e-3, (name, k, "restart taken without optimize_b", float(parsg), g_first, parsr)
    assert d_g <= PARS_ATOL, (name, k, float(parsg), parsr)                         # observed 3.3e-8
    e_c, e_raw = rel(Cg, Cr), rel(Crawg, Crawr)
    assert e_c <= C_TOL, (name, k, e_c)                                             # observed 2.8e-7
    assert e_raw <= C_RAW_TOL, (name, k, e_raw)                                     # observed 8.2e-8
    assert np.array_equal(Sg > 0, Sr > 0), (name, k, np.nonzero((Sg > 0) != (Sr > 0))[0][:8])
    e_s = rel(Sg, Sr) if Sr.any() else 0.0
    assert e_s <= S_TOL, (name, k, e_s)                                             # observed 1.7e-7
    return dict(sn=d_sn, pars=d_g, C=e_c, C_raw=e_raw, S=e_s)


@pytest.mark.parametrize("case", dbc.all_cases(), ids=lambda c: c[0])
def test_deconv_branch_case(eng, observed, case):
    import oasis_oracle as oo
    name, Y, opts, tags = case
    ref = dbc.reference(name)
    got = eng.deconv_temporal(Y, dict(opts, type="ar1", method="foopsi"))
    family = name.split("_")[0]
    for k, tag in enumerate(tags):
        g_first = None
        if tag in ("restart", "update_g"):
            y = Y[k].astype(np.float64)
            g_first = oo.estimate_time_constant_ar1(y, oo.GetSn(y))
        fig = _compare_row(name, k, tag, Y[k], [a[k] for a in got], [a[k] for a in ref], g_first)
        if fig:
            print("%s row %d (%s): %s" % (name, k, tag, " ".join("%s %.2e" % kv for kv in fig.items())))
            _note(observed, family, **fig)


def test_hals_sweep_with_restart(eng, observed):
    """the fused path (hals_temporal_deconv, two sweeps, max_tau = 5): the median's ties, the restart's GetSn on the row HALS_temporal.m:88 took b off, and the
    preset pars of sweep 2 (which exceed gmax again: a second restart) against oo.HALS_temporal_deconv on the exported residual"""
    import oasis_oracle as oo
    from cnmf_e_amd import synth
    from cnmf_e_amd.sources2d import PatchedVideo
    h = dbc.HALS
    f = synth.make_factors(h["d1"], h["d2"], h["T"], h["K"], h["seed"], gSig=1.5, gSiz=7, min_sep=5)
    Yv = synth.make_video(f, np.float32)
    video = PatchedVideo(h["d1"], h["d2"], h["T"], [h["d1"], h["d2"]], h["r"], eng)
    video.upload_from_full(Yv)
    pid = video.pid[video.order[0]]
    eng.ring_init(pid, h["r"])
    eng.fit_ring_model(pid, None, None)
    ysig = eng.residual(pid, None, None, want=True).T.astype(np.float64)
    A_p = f.A_true.tocsc().astype(np.float32)
    o = {k: v for k, v in h["opts"].items()}
    Cg, Crawg, Sg, sng, parsg, aa = eng.hals_temporal_deconv(pid, A_p, f.C_init, h["sweeps"], dict(o, type="ar1", method="foopsi"))
    Cr, Crawr, Sr, snr, parsr = oo.HALS_temporal_deconv(ysig, A_p.astype(np.float64), f.C_init, h["sweeps"], **o)
    parsr = np.array(parsr, dtype=np.float64)
    # branch reached: gamma after one sweep exceeds gmax on most rows (three of four here), so their sweep 2 starts from a preset gamma and restarts
    # (foopsi_oasisAR1.m:104-108); a row below gmax runs update_g from its preset gamma instead
    pars1 = np.array(oo.HALS_temporal_deconv(ysig, A_p.astype(np.float64), f.C_init, 1, **o)[4], dtype=np.float64)
    assert (pars1 > dbc.GMAX5).sum() >= 2 and ((pars1 > 0) & (pars1 <= dbc.GMAX5)).sum() >= 1, pars1
    # well-conditioned: every GetSn of the oracle scaled by 1 +- 1e-6 keeps the support and moves gamma and C by < 1e-5
    get_sn = oo.GetSn
    try:
        for fct in (1 - 1e-6, 1 + 1e-6):
            oo.GetSn = lambda y, _f=fct: get_sn(y) * _f
            C2, _, S2, _, pars2 = oo.HALS_temporal_deconv(ysig, A_p.astype(np.float64), f.C_init, h["sweeps"], **o)
            assert np.array_equal(S2 > 0, Sr > 0)
            assert np.abs(np.array(pars2, dtype=np.float64) - parsr).max() < 1e-5 and np.linalg.norm(C2 - Cr) / np.linalg.norm(Cr) < 1e-5
    finally:
        oo.GetSn = get_sn
    print("hals: sn %s\n      pars engine %s\n      pars oracle %s" % (np.abs(sng / snr - 1), parsg, parsr))
    assert np.allclose(sng, snr, rtol=SN_RTOL, atol=0)                              # observed 9.5e-8
    assert np.allclose(parsg, parsr, rtol=0, atol=PARS_ATOL), (parsg, parsr)        # observed 1.4e-7 (with GetSn of y instead of y - b in the restart: 1.2e-3)
    for k in range(h["K"]):
        e_c, e_raw = rel(Cg[k], Cr[k]), rel(Crawg[k], Crawr[k])
        assert np.array_equal(Sg[k] > 0, Sr[k] > 0), (k, np.nonzero((Sg[k] > 0) != (Sr[k] > 0))[0][:8])
        e_s = rel(Sg[k], Sr[k]) if Sr[k].any() else 0.0
        print("hals row %d: pars %.2e C %.2e C_raw %.2e S %.2e" % (k, abs(parsg[k] - parsr[k]), e_c, e_raw, e_s))
        _note(observed, "hals", sn=abs(sng[k] / snr[k] - 1), pars=abs(parsg[k] - parsr[k]), C=e_c, C_raw=e_raw, S=e_s)
        assert e_c <= C_TOL and e_raw <= C_RAW_TOL, (k, e_c, e_raw)                 # observed 7.9e-8, 9.3e-8
        assert e_s <= S_TOL, (k, e_s)                                               # observed 7.3e-8
