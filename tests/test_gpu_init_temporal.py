"""initTemporal on the device (cnmfe_init_temporal[_job], cnmf_e_amd/csrc/init_temporal.hpp; Sources2D.initTemporal / set_W / set_b0) against the float64
restatement of @Sources2D/initTemporal.m (tests/init_temporal_oracle.py) on the fixtures of tests/init_temporal_cases.py.

Tolerances follow the rule of tests/test_gpu_parity.py: 10 x the error observed on the MI355X, rounded up to one digit, never above 1e-4 (DESIGN.md section 8
lists the observed values; the `observed` fixture records them again in every run).  The deconvolved quantities of case B take the bounds
test_hals_temporal_deconv_parity asserts: traces 5e-6 relative Frobenius, gamma 2e-6 absolute."""
import os
import sys

import numpy as np
import pytest
import scipy.sparse as sp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
pytestmark = pytest.mark.gpu

from parity_util import rel

# 10 x observed, one digit, <= 1e-4.  Observed on the MI355X ("(f) known footprints"): A 6.5e-8 (9.9e-8 on the int8 pipe after a fit),
# C 8.1e-8 (1.0e-7), C with the empty column 7.7e-8, D 4.3e-6 (80 footprints one pixel apart: V is close to singular), B's plain sweeps 8.1e-8
TOL = {"A": 1e-6, "C": 2e-6, "D": 5e-5, "B_plain_patch": 9e-7}
TRACE_B, GAMMA_B = 5e-6, 2e-6


class Run:
    def __init__(self, name, lanes=1, A=None, **opt):
        import init_temporal_cases as itc
        from cnmf_e_amd.engine import Engine
        from cnmf_e_amd.sources2d import PatchedVideo, Sources2D, Options
        self.c = c = itc.make(name)
        self.eng = Engine(0)
        if lanes > 1:
            self.eng.set_option("lanes", lanes)
        self.video = PatchedVideo(c.d1, c.d2, c.T, c.pdims, c.r, self.eng)
        self.video.upload_from_full(c.Y)
        A = c.A if A is None else A
        self.s = Sources2D(self.video, Options(ring_radius=c.r, deconv_flag=c.deconv is not None, deconv_options=c.deconv or {}, **opt), A,
                           np.zeros((A.shape[1], c.T), np.float32), np.ones(c.d1 * c.d2, np.float32))
        for idx in self.video.owned:
            self.s.set_W(idx, c.W[idx]); self.s.set_b0(idx, c.b0[idx])

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.eng.close()


def _calls(eng):
    return {k: v["calls"] for k, v in eng.profile_table().items() if v["calls"]}


@pytest.mark.parametrize("name,passes", [("A", 1), ("C", 1), ("D", 3)])
def test_plain_parity(name, passes, observed):
    """C_raw = C against the oracle; two calls are bit-equal; one projection launch set per patch with neurons (case D: a 16 x 16 block meets 160 columns of
    (E - W)' [At, tmp_A], the 64 slots of a panel list take them in three passes); a following update_background_parallel uploads no K x T matrix"""
    import init_temporal_cases as itc
    ref = itc.reference(name)
    with Run(name) as r:
        s, eng = r.s, r.eng
        for idx in r.video.owned:                            # the transplanted background is what the device holds, and it counts as fitted
            assert rel(s.get_W(idx).toarray(), r.c.W[idx].toarray()) == 0 and np.array_equal(s.get_b0(idx), r.c.b0[idx])
            assert not eng.ring_first_run(r.video.pid[idx])
        eng.profile(True)
        s.initTemporal()
        calls = _calls(eng)
        eng.profile(False)
        C1 = np.asarray(s.C_raw, dtype=np.float32).copy()
        assert s.C is s.C_raw and not np.isnan(C1).any()
        e = rel(C1, ref["C_raw"])
        observed["init_temporal_%s_C_raw" % name] = e
        print("init_temporal %s: rel(C_raw) = %.3g, levels %d" % (name, e, eng.counter("init_temporal_levels")))
        assert e <= TOL[name], e
        npatch = sum(1 for ind in ref["ind"].values() if ind.size)
        assert calls.get("temporal_build_B") == npatch * passes and calls.get("init_temporal_filter") == npatch, calls
        assert not ({"temporal_proj_U", "residual_r1", "residual_r1_generic"} & set(calls)), sorted(calls)
        for k in range(r.c.K if name != "D" else 0):
            assert np.corrcoef(C1[k], r.c.C_true[k])[0, 1] > 0.85, k
        s.initTemporal()                                      # two calls are bit-equal
        assert np.array_equal(np.asarray(s.C_raw, dtype=np.float32), C1)
        # the new traces are the bound matrix: the next background fit reads them where they lie
        up0 = eng.counter("trace_matrix_uploads")
        s.update_background_parallel()
        assert eng.counter("trace_matrix_uploads") == up0
        # the fit leaves the video's digit planes resident: the projection then runs on the int8 pipe (other bits, the same bound).  The fit changed W:
        # the fixture's goes back first
        for idx in r.video.owned:
            s.set_W(idx, r.c.W[idx]); s.set_b0(idx, r.c.b0[idx])
        s.initTemporal()
        e8 = rel(np.asarray(s.C_raw, dtype=np.float32), ref["C_raw"])
        observed["init_temporal_%s_C_raw_after_fit" % name] = e8
        print("init_temporal %s after a fit: rel(C_raw) = %.3g" % (name, e8))
        assert e8 <= TOL[name], e8


def test_lanes_bit_equal():
    with Run("A") as r1:
        r1.s.initTemporal()
        C1 = np.asarray(r1.s.C_raw, dtype=np.float32).copy()
    with Run("A", lanes=2) as r2:
        assert r2.eng.counter("lanes_live") == 2
        r2.s.initTemporal()
        assert np.array_equal(np.asarray(r2.s.C_raw, dtype=np.float32), C1)


def _deconv_run(observed):
    """case B through the patch call and through the method, with every error against the oracle"""
    import init_temporal_cases as itc
    import init_temporal_oracle as ito
    ref = itc.reference("B")
    pp = ref["per_patch"][(0, 0)]
    with Run("B") as r:
        s, eng, c = r.s, r.eng, r.c
        idx = r.video.owned[0]; pid = r.video.pid[idx]
        A_blk = sp.csc_matrix(c.A)[r.video.block_pix[idx]]
        # the twelve sweeps without deconvolution: the projection, V and the schedule of this geometry (r = 8)
        _, Crp, _, _, _, AA = eng.init_temporal(pid, A_blk, 10, 2, None)
        plain = ito.init_temporal_patch(c.Y[:, r.video.block_pix[idx]].T, A_blk, c.W[idx], np.isin(r.video.block_pix[idx], r.video.patch_pix[idx]), None)
        errs = dict(plain_C_raw=rel(Crp, plain["C_raw"]))
        assert np.allclose(AA, pp["AA"], rtol=1e-6)
        first = eng.init_temporal(pid, A_blk, 10, 2, c.deconv)
        Cg, Crg, Sg, kp, sn, _ = first
        errs.update(C=max(rel(Cg[k], pp["C"][k]) for k in range(c.K)), C_raw=max(rel(Crg[k], pp["C_raw"][k]) for k in range(c.K)),
                    S=max(rel(Sg[k], pp["S"][k]) for k in range(c.K)), gamma=float(np.max(np.abs(kp - pp["kernel_pars"]))), sn=float(np.max(np.abs(sn / pp["sn"] - 1))))
        second = eng.init_temporal(pid, A_blk, 10, 2, c.deconv)
        s.initTemporal()
        errs.update(m_C=max(rel(np.asarray(s.C)[k], ref["C"][k]) for k in range(c.K)), m_C_raw=max(rel(np.asarray(s.C_raw)[k], ref["C_raw"][k]) for k in range(c.K)),
                    m_S=max(rel(np.asarray(s.S)[k], ref["S"][k]) for k in range(c.K)),
                    m_gamma=float(np.max(np.abs(np.asarray(s.P["kernel_pars"]).ravel() - ref["kernel_pars"]))),
                    m_sn=float(np.max(np.abs(np.asarray(s.P["neuron_sn"]).ravel() / ref["neuron_sn"] - 1))))
        for k, v in errs.items():
            observed["init_temporal_B_%s" % k] = v
        print("init_temporal B:", {k: "%.3g" % v for k, v in errs.items()})
        return errs, first, second, (np.asarray(s.C).copy(), np.asarray(s.C_raw).copy(), np.asarray(s.S).copy()), c


def test_deconv_runs(observed):
    """case B, deconv_flag: two patch calls are bit-equal, nothing is NaN, the plain sweeps of this geometry and the in-sweep noise levels match the oracle --
    sn includes what the raw video's offset leaks into Welch's band (HALS_temporal.m:79 before :88), so the per-row constant the deconvolution kernel adds
    where GetSn reads the row is the reference's --, and the method recovers the planted traces"""
    errs, first, second, (Cm, Crm, Sm), c = _deconv_run(observed)
    for a, b in zip(first[:5], second[:5]):
        assert np.array_equal(a, b)
    assert not any(np.isnan(np.asarray(x)).any() for x in first[:5] + (Cm, Crm, Sm))
    assert errs["plain_C_raw"] <= TOL["B_plain_patch"], errs
    assert errs["sn"] <= 2e-5 and errs["m_sn"] <= 7e-7, errs                      # observed 1.9e-6 (fp32 Welch transform of a row thousands above its signal) and, after deconvTemporal, 6.2e-8: 10 x
    assert np.all(Sm >= 0)
    for k in range(c.K):
        assert np.corrcoef(Cm[k], c.C_true[k])[0, 1] > 0.9


def test_deconv_parity(observed):
    """case B against the oracle at the bounds test_hals_temporal_deconv_parity asserts: traces 5e-6 relative Frobenius, gamma 2e-6 absolute.

    Observed on the MI355X: the patch call's in-sweep results C 5.8e-8, C_raw 8.1e-8, gamma 3.1e-8 (S: both sides all zero), the method's (after deconvTemporal)
    C 5.6e-8, C_raw 7.7e-8, S 7.6e-8, gamma 2.9e-8.  The reference regresses the RAW video, so a row update lies 500 .. 3000 above its signal here (the fitted W
    has an intercept: (E - W) Ymean is hundreds per pixel), and GetSn is taken before the baseline goes.  The engine keeps U centred and hands the deconvolution
    kernel that constant per row in fp64, for GetSn alone; foopsi's g > gmax restart (foopsi_oasisAR1.m:105) takes GetSn of the baseline-subtracted row, as the
    reference does.  (With the constant inside the fp32 row the traces missed the bound at 7e-6 .. 3e-5, and with the restart's GetSn on the row with its offset the
    in-sweep gamma was off by 0.80.)"""
    errs, *_ = _deconv_run(observed)
    assert errs["m_C"] <= TRACE_B and errs["m_C_raw"] <= TRACE_B and errs["m_S"] <= TRACE_B and errs["m_gamma"] <= GAMMA_B, errs
    assert errs["C"] <= TRACE_B and errs["C_raw"] <= TRACE_B and errs["S"] <= TRACE_B and errs["gamma"] <= GAMMA_B, errs


def test_deconv_jobs_equal_patch_calls():
    """case A's four patches with case B's deconvolution options: the job form (one launch per level over all patches, each job with its own per-row GetSn offsets)
    gives the bits of the patch-by-patch form, whose in-sweep results test_deconv_parity holds against the oracle"""
    import init_temporal_cases as itc
    dopt = itc.make("B").deconv
    got = []
    for jobs in (True, False):
        with Run("A") as r:
            r.s.options.deconv_flag, r.s.options.deconv_options = True, dopt
            assert r.eng.supports_temporal_jobs
            if not jobs:
                r.eng.supports_temporal_jobs = False              # (the instance only: Sources2D then calls cnmfe_init_temporal patch by patch)
            r.eng.profile(True)
            r.s.initTemporal()
            calls = _calls(r.eng)
            r.eng.profile(False)
            assert calls.get("temporal_hals_deconv_level"), calls
            got.append([np.asarray(x, dtype=np.float32).copy() for x in (r.s.C, r.s.C_raw, r.s.S, np.asarray(r.s.P["kernel_pars"]).ravel(), np.asarray(r.s.P["neuron_sn"]).ravel())])
    for a, b in zip(*got):
        assert not np.isnan(a).any() and np.array_equal(a, b)
    assert got[0][1].any()


def test_empty_footprint_stays_zero(observed):
    """case C with a fourth, empty footprint: its aa = 0 row is never updated and stays at the rough start's zero; nothing is NaN"""
    import init_temporal_cases as itc
    import init_temporal_oracle as ito
    c = itc.make("C")
    A4 = sp.hstack([c.A, sp.csc_matrix((c.d1 * c.d2, 1), dtype=np.float32)]).tocsc()
    with Run("C", A=A4) as r:
        idx = r.video.owned[0]; pid = r.video.pid[idx]
        Cg, Crg, _, _, _, AA = r.eng.init_temporal(pid, A4, 10, 2, None)          # (one patch = the field of view: block rows are FOV pixels)
        want = ito.init_temporal_patch(c.Y.T, A4, c.W[idx], np.ones(c.d1 * c.d2, bool), None)
        assert not np.isnan(Cg).any() and not np.isnan(Crg).any()
        assert not Cg[3].any() and not Crg[3].any() and AA[3] == 0 and not want["C_raw"][3].any()
        e = rel(Crg, want["C_raw"])
        observed["init_temporal_C4_C_raw"] = e
        assert e <= TOL["C"] and np.array_equal(Cg, Crg)
        r.s.initTemporal()
        Cm = np.asarray(r.s.C_raw)
        assert Cm.shape == (4, c.T) and not Cm[3].any() and not np.isnan(Cm).any() and rel(Cm[:3], itc.reference("C")["C_raw"]) <= TOL["C"]


def test_refusals_leave_no_state():
    from cnmf_e_amd import _lib as L
    with Run("C") as r:
        s, eng, c = r.s, r.eng, r.c
        idx = r.video.owned[0]; pid = r.video.pid[idx]
        s.initTemporal()
        C1 = np.asarray(s.C_raw, dtype=np.float32).copy()
        held = (s.C, s.C_raw)
        # a derived (bg_ssub) patch: CNMFE_EUNSUPPORTED; a patch without a ring: CNMFE_ESTATE; no footprints: CNMFE_EINVAL
        eng.patch_derive(pid, 7, 2, "nearest")
        eng.ring_init(7, 4)
        low = sp.csc_matrix(np.ones((eng._patch[7]["d_b"], 1), np.float32))
        with pytest.raises(L.CnmfeError, match="error -5"):
            eng.init_temporal(7, low)
        eng.create_patch(9, [1, c.d1, 1, c.d2], [1, c.d1, 1, c.d2], c.d1, c.d2, c.T)
        eng.upload_block(9, c.Y)
        with pytest.raises(L.CnmfeError, match="error -4"):
            eng.init_temporal(9, c.A)
        with pytest.raises(L.CnmfeError, match="error -1"):
            eng.init_temporal(pid, sp.csc_matrix((c.d1 * c.d2, 0), dtype=np.float32))
        s.ssub = 2
        with pytest.raises(NotImplementedError):
            s.initTemporal()
        s.ssub = 1
        A_keep, s.A = s.A, sp.csc_matrix((c.d1 * c.d2, 0), dtype=np.float32)
        with pytest.raises(ValueError):
            s.initTemporal()
        s.A = A_keep
        assert s.C is held[0] and s.C_raw is held[1]
        s.initTemporal()                                      # ... and the next call computes what the first did
        assert np.array_equal(np.asarray(s.C_raw, dtype=np.float32), C1)
