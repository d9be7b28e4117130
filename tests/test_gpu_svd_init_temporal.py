"""initTemporal under background_model = 'svd' on the device (cnmfe_init_temporal_lowrank, cnmf_e_amd/csrc/init_temporal_lowrank.hpp; Sources2D.initTemporal) against
the float64 restatement of @Sources2D/initTemporal.m:180-192 (tests/svd_init_temporal_oracle.py) on the fixtures of tests/svd_init_temporal_cases.py.

Tolerances follow the rule of tests/test_gpu_parity.py: at most 10 x the error observed on the MI355X, and no plain-sweep bound above 5e-5, the loosest plain bound
of the ring branch's test (DESIGN.md section 8 and profiles/svd_init_temporal/probe.json list the observed values; the `observed` fixture records them again in every
run).  The deconvolved quantities of case a take the bounds test_gpu_init_temporal.py::test_deconv_parity asserts: traces 5e-6 relative Frobenius, gamma 2e-6 absolute."""
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

# Observed on the MI355X ("(f) known footprints under the low-rank background"), maxima over the patches of a case, relative Frobenius:
#   C_raw              a 8.7e-8, b 1.6e-7, c 1.7e-6 (80 footprints one pixel apart), d 6.3e-8, e 1.1e-7, f 7.9e-8: one fp32 rounding of U and of the start, then twelve
#                      fp32 sweeps.  Every bound is 10 x its value, all below the 5e-5 of the ring branch's test
#   f, stored video    a 1.0e-15, b 2.0e-15, c 1.5e-15, e 1.0e-15, f 9.3e-16: against the oracle run on the video AS THE ENGINE STORES IT (svd_init_temporal_oracle.
#                      stored_video: centred in float32, which rounds where a sample is more than a factor 2 from its pixel's mean).  This is the arithmetic of the
#                      Gram matrix, the projection, the factorisation and the solve: float64 throughout
#   f, the recording   a 1.1e-9, b 2.0e-9, c 2.9e-9, e 1.4e-9, f 7.5e-10: the same f against the oracle on the float32 recording itself.  The difference to the line
#                      above is that input rounding of the RESIDENT video (2^-24 of a sample, averaged over the patch's pixels), not arithmetic: nothing behind the
#                      upload can undo it
#   b0                 exact: the float64 mean of T float32 samples has one value whatever the order of the sum
TOL_C = {"a": 8.7e-7, "b": 1.5e-6, "c": 1.6e-5, "d": 6.2e-7, "e": 1.1e-6, "f": 7.8e-7}
TOL_F = {"a": 1.0e-8, "b": 1.9e-8, "c": 2.8e-8, "e": 1.4e-8, "f": 7.4e-9}
TOL_F_STORED = 1.9e-14
TRACE_A, GAMMA_A = 5e-6, 2e-6
PASSES = {"a": 1, "b": 1, "c": 2, "d": 1, "e": 1}           # projection passes of a patch with neurons (c: 88 columns over one 16 x 16 block, 64 list slots)


class Run:
    def __init__(self, name, deconv=False, A=None):
        import svd_init_temporal_cases as sic
        from cnmf_e_amd.engine import Engine
        from cnmf_e_amd.sources2d import PatchedVideo, Sources2D, Options
        self.c = c = sic.make(name)
        self.eng = Engine(0)
        self.video = PatchedVideo(c.d1, c.d2, c.T, c.pdims, c.halo, self.eng)
        self.video.upload_from_full(c.Y)
        A = c.A if A is None else A
        self.s = Sources2D(self.video, Options(background_model="svd", nb=c.nb, ring_radius=c.halo, deconv_flag=deconv, deconv_options=dict(sic.DECONV) if deconv else {}),
                           A, np.zeros((A.shape[1], c.T), np.float32), np.ones(c.d1 * c.d2, np.float32))
        self.transplant()

    def transplant(self):
        c = self.c
        for idx in self.video.owned:
            self.s.set_bg_svd(idx, c.b[idx], np.zeros((c.nb, c.T)), np.zeros(c.b[idx].shape[0]))

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.eng.close()


def _calls(eng):
    return {k: v["calls"] for k, v in eng.profile_table().items() if v["calls"]}


def _factor_errors(r, ref):
    """max over the patches with neurons of rel(f) against the oracle on the recording and on the stored video, and |b0 - b0_ref| / max |b0_ref|: the engine's
    resident factors against the oracle's"""
    import svd_init_temporal_oracle as sio
    ef = eb = es = 0.0
    for idx in r.video.owned:
        if ref["f"][idx] is None:
            continue
        f, b0 = r.s.get_f(idx), r.s.get_b0(idx)
        assert f.shape == ref["f"][idx].shape and np.array_equal(r.s.get_b(idx), r.c.b[idx])
        if f.size:
            ef = max(ef, rel(f, ref["f"][idx]))
            pp = r.video.patch_pix[idx]
            Ys, m = sio.stored_video(r.c.Y[:, pp].T)
            es = max(es, rel(f, sio.init_temporal_patch(Ys, r.c.A.toarray()[pp][:, ref["ind"][idx]], r.c.b[idx], b0=m, iters=(0, 0))["f"]))
        eb = max(eb, float(np.abs(b0 - ref["b0"][idx]).max() / np.abs(ref["b0"][idx]).max()))
    return ef, es, eb


@pytest.mark.parametrize("name", ["a", "b", "c", "d", "e"])
def test_plain_parity(name, observed):
    """C_raw = C, f and b0 against the oracle; two calls are bit-equal; the video is read once per projection pass; the update_temporal_parallel that follows
    uploads no K x T matrix"""
    import svd_init_temporal_cases as sic
    ref = sic.reference(name)
    with Run(name) as r:
        s, eng, c = r.s, r.eng, r.c
        eng.profile(True)
        s.initTemporal()
        calls = _calls(eng)
        eng.profile(False)
        C1 = np.asarray(s.C_raw, dtype=np.float32).copy()
        assert s.C is s.C_raw and np.isfinite(C1).all()
        e = rel(C1, ref["C_raw"])
        ef, es, eb = _factor_errors(r, ref)
        observed["svd_init_temporal_%s" % name] = dict(C_raw=e, f=ef, f_stored=es, b0=eb)
        print("svd init_temporal %s: rel(C_raw) = %.3g, rel(f) = %.3g (stored video: %.3g), b0 = %.3g" % (name, e, ef, es, eb))
        assert e <= TOL_C[name], e
        assert eb == 0 and (c.nb == 0 or (ef <= TOL_F[name] and es <= TOL_F_STORED)), (ef, es, eb)
        for idx in r.video.owned:                            # a dropped column's row of f is exactly 0
            if ref["f"][idx] is not None:
                for i in c.zero_cols:
                    assert not s.get_f(idx)[i].any()
        npatch = sum(1 for ind in ref["ind"].values() if ind.size)
        assert eng.counter("init_temporal_lowrank_video_reads") == PASSES[name]
        assert calls.get("temporal_build_B") == npatch * PASSES[name] and calls.get("itl_trsm_forward") == npatch and calls.get("itl_trsm_backward") == npatch, calls
        assert not ({"lowrank_resid", "temporal_proj_U", "init_temporal_filter"} & set(calls)), sorted(calls)      # no Ysig is formed, no ring is read
        for k in range(c.K if name != "c" else 0):
            if c.C_true[k].any():                            # (a planted trace without a spike in these frames has nothing to correlate with)
                assert np.corrcoef(C1[k], c.C_true[k])[0, 1] > 0.9, k
        fb = {idx: (s.get_f(idx).copy(), s.get_b0(idx).copy()) for idx in r.video.owned}
        s.initTemporal()                                      # two calls are bit-equal: f and b0 went in as part of the state and come out the same
        assert np.array_equal(np.asarray(s.C_raw, dtype=np.float32), C1)
        for idx in r.video.owned:
            assert np.array_equal(s.get_f(idx), fb[idx][0]) and np.array_equal(s.get_b0(idx), fb[idx][1])
        # the new traces are the bound matrix: the temporal update reads them where they lie
        up0 = eng.counter("trace_matrix_uploads")
        s.update_temporal_parallel()
        assert eng.counter("trace_matrix_uploads") == up0
        assert np.isfinite(np.asarray(s.C_raw)).all()


def test_patch_call_reports_what_it_leaves(observed):
    """the patch call on case b's fullest patch (n = 18: two 16-tiles, the second one mostly padding): its outputs against the oracle's patch, f and b0 as reported
    are what cnmfe_bg_svd_get returns afterwards, AA is the diagonal of A'A on the patch, and the patch is in the state of a set: no resident Ysig"""
    import svd_init_temporal_cases as sic
    from cnmf_e_amd import _lib as L
    ref = sic.reference("b")
    with Run("b") as r:
        eng, c, v = r.eng, r.c, r.video
        idx = (0, 0); pid = v.pid[idx]
        ind = ref["ind"][idx]
        assert ind.size + c.nb == 18
        A_blk = sp.csc_matrix(c.A)[v.block_pix[idx]][:, ind]
        eng.residual_lowrank(pid)                             # a resident Ysig of the OLD factors ...
        Cg, Crg, S, kp, sn, AA, f, b0 = eng.init_temporal_lowrank(pid, A_blk, 10, 2, None)
        pp = ref["per_patch"][idx]
        assert S is None and kp is None and sn is None
        e = dict(C=rel(Cg, pp["C"]), C_raw=rel(Crg, pp["C_raw"]), f=rel(f, pp["f"]), AA=float(np.abs(AA / pp["AA"] - 1).max()))
        observed["svd_init_temporal_b_patch"] = e
        print("svd init_temporal b, patch (0, 0):", {k: "%.3g" % x for k, x in e.items()})
        assert e["C"] <= TOL_C["b"] and e["C_raw"] <= TOL_C["b"] and e["f"] <= TOL_F["b"] and e["AA"] <= 1.2e-7      # (AA: one fp32 rounding)
        assert np.array_equal(b0, pp["b0"])
        bg, fg, b0g = eng.bg_svd_get(pid)
        assert np.array_equal(fg, f) and np.array_equal(b0g, b0) and np.array_equal(bg, c.b[idx])
        with pytest.raises(L.CnmfeError, match="error -4"):  # ... is invalid afterwards: an update asks for a fresh one
            eng.hals_temporal(pid, sp.csc_matrix(c.A)[v.patch_pix[idx]][:, ind], Cg, 2)


def test_deconv_parity(observed):
    """case a with deconv_flag, compared as tests/test_gpu_init_temporal.py::test_deconv_parity compares: every trace's relative Frobenius error and gamma's absolute
    error, for the patch calls' in-sweep results and for the method's (after deconvTemporal); two patch calls are bit-equal"""
    import svd_init_temporal_cases as sic
    ref = sic.reference("a", True)
    with Run("a", deconv=True) as r:
        s, eng, c, v = r.s, r.eng, r.c, r.video
        errs = dict(C=0.0, C_raw=0.0, S=0.0, gamma=0.0, sn=0.0)
        for idx in v.owned:
            ind = ref["ind"][idx]
            pp = ref["per_patch"][idx]
            A_blk = sp.csc_matrix(c.A)[v.block_pix[idx]][:, ind]
            first = eng.init_temporal_lowrank(v.pid[idx], A_blk, 10, 2, s.options.deconv_options)
            Cg, Crg, Sg, kp, sn = first[:5]
            assert all(np.isfinite(np.asarray(x)).all() for x in first)
            for k in range(ind.size):
                errs["C"] = max(errs["C"], rel(Cg[k], pp["C"][k])); errs["C_raw"] = max(errs["C_raw"], rel(Crg[k], pp["C_raw"][k]))
                if pp["S"][k].any() or Sg[k].any():
                    errs["S"] = max(errs["S"], rel(Sg[k], pp["S"][k]))
            errs["gamma"] = max(errs["gamma"], float(np.max(np.abs(kp - pp["kernel_pars"]))))
            errs["sn"] = max(errs["sn"], float(np.max(np.abs(sn / pp["sn"] - 1))))
            r.transplant()
            second = eng.init_temporal_lowrank(v.pid[idx], A_blk, 10, 2, s.options.deconv_options)
            assert all(np.array_equal(a, b) for a, b in zip(first, second))
        r.transplant()
        s.initTemporal()
        errs.update(m_C=max(rel(np.asarray(s.C)[k], ref["C"][k]) for k in range(c.K)), m_C_raw=max(rel(np.asarray(s.C_raw)[k], ref["C_raw"][k]) for k in range(c.K)),
                    m_S=max(rel(np.asarray(s.S)[k], ref["S"][k]) for k in range(c.K)),
                    m_gamma=float(np.max(np.abs(np.asarray(s.P["kernel_pars"]).ravel() - ref["kernel_pars"]))),
                    m_sn=float(np.max(np.abs(np.asarray(s.P["neuron_sn"]).ravel() / ref["neuron_sn"] - 1))))
        for k, x in errs.items():
            observed["svd_init_temporal_a_deconv_%s" % k] = x
        print("svd init_temporal a, deconvolution:", {k: "%.3g" % x for k, x in errs.items()})
        assert errs["m_C"] <= TRACE_A and errs["m_C_raw"] <= TRACE_A and errs["m_S"] <= TRACE_A and errs["m_gamma"] <= GAMMA_A, errs
        assert errs["C"] <= TRACE_A and errs["C_raw"] <= TRACE_A and errs["S"] <= TRACE_A and errs["gamma"] <= GAMMA_A, errs
        assert np.all(np.asarray(s.S) >= 0)
        for k in range(c.K):
            assert np.corrcoef(np.asarray(s.C)[k], c.C_true[k])[0, 1] > 0.9


def test_patch_without_neurons_keeps_its_factors():
    """case f: the lower right patch has no neuron; its b, f, b0 are bit for bit what they were (initTemporal.m:156-159), the others' f and b0 are new"""
    import svd_init_temporal_cases as sic
    ref = sic.reference("f")
    with Run("f") as r:
        s, c, v = r.s, r.c, r.video
        rng = np.random.default_rng(5)
        empty = (1, 1)
        n = v.patch_pix[empty].size
        mine = (c.b[empty], rng.normal(size=(c.nb, c.T)), rng.normal(size=n))
        s.set_bg_svd(empty, *mine)
        s.initTemporal()
        assert np.array_equal(s.get_b(empty), mine[0]) and np.array_equal(s.get_f(empty), mine[1]) and np.array_equal(s.get_b0(empty), mine[2])
        for idx in v.owned:
            if idx != empty:
                assert s.get_f(idx).any() and rel(s.get_f(idx), ref["f"][idx]) <= TOL_F["f"]
        e = rel(np.asarray(s.C_raw), ref["C_raw"])
        print("svd init_temporal f: rel(C_raw) = %.3g" % e)
        assert e <= TOL_C["f"], e


def test_refusals_leave_no_state():
    """no factors: CNMFE_ESTATE; two identical footprints: a Cholesky pivot at rounding level, the message names the patch and the pivot; more unknowns than the cap
    (option init_temporal_lowrank_nmax stands in for 2048): CNMFE_EUNSUPPORTED.  None of them changes f, b0, the resident residual or the traces, and the next good
    call computes what the first did."""
    import svd_init_temporal_cases as sic
    from cnmf_e_amd import _lib as L
    with Run("a") as r:
        s, eng, c, v = r.s, r.eng, r.c, r.video
        idx = (0, 0); pid = v.pid[idx]
        s.initTemporal()
        C1 = np.asarray(s.C_raw, dtype=np.float32).copy()
        held = (s.C, s.C_raw)
        f1, b01 = s.get_f(idx).copy(), s.get_b0(idx).copy()
        Ysig1 = eng.residual_lowrank(pid, want=True).copy()
        ind = sic.reference("a")["ind"][idx]
        A_blk = sp.csc_matrix(c.A)[v.block_pix[idx]][:, ind]
        twins = sp.hstack([A_blk, A_blk[:, :1]]).tocsc()
        with pytest.raises(L.CnmfeError, match=r"error -4.*patch %d.*pivot %d" % (pid, ind.size)):
            eng.init_temporal_lowrank(pid, twins)
        eng.set_option("init_temporal_lowrank_nmax", ind.size)            # k + nb = k + 1 unknowns: one too many
        with pytest.raises(L.CnmfeError, match="error -5"):
            eng.init_temporal_lowrank(pid, A_blk)
        eng.set_option("init_temporal_lowrank_nmax", 2048)
        with pytest.raises(L.CnmfeError, match="error -1"):
            eng.init_temporal_lowrank(pid, sp.csc_matrix((v.block_pix[idx].size, 0), dtype=np.float32))
        eng.create_patch(9, [1, c.d1, 1, c.d2], [1, c.d1, 1, c.d2], c.d1, c.d2, c.T)
        eng.upload_block(9, c.Y)
        with pytest.raises(L.CnmfeError, match="error -4"):               # no fit, no set
            eng.init_temporal_lowrank(9, c.A)
        assert np.array_equal(s.get_f(idx), f1) and np.array_equal(s.get_b0(idx), b01)
        up0 = eng.counter("trace_matrix_uploads")
        eng.profile(True)
        n0 = _calls(eng).get("lowrank_resid", 0)
        assert np.array_equal(eng.residual_lowrank(pid, want=True), Ysig1)          # still resident: nothing is swept again
        assert _calls(eng).get("lowrank_resid", 0) == n0
        eng.profile(False)
        assert s.C is held[0] and s.C_raw is held[1] and eng.counter("trace_matrix_uploads") == up0
        r.transplant()
        s.initTemporal()
        assert np.array_equal(np.asarray(s.C_raw, dtype=np.float32), C1)


def test_own_fit_keeps_the_refusal_until_the_factors_are_handed_back():
    """after this object's own update_background_parallel initTemporal stays refused, as before the branch was built (tests/test_gpu_svd_bg.py pins that on the real
    engine); set_bg_svd with the fitted factors lifts it, and the call then runs under exactly that b"""
    with Run("a") as r:
        s, v = r.s, r.video
        s.initTemporal()
        s.update_background_parallel()
        with pytest.raises(NotImplementedError, match="svd"):
            s.initTemporal()
        fitted = {idx: (s.get_b(idx), s.get_f(idx), s.get_b0(idx)) for idx in v.owned}
        for idx in v.owned:
            s.set_bg_svd(idx, *fitted[idx])
        s.initTemporal()
        assert np.isfinite(np.asarray(s.C_raw)).all()
        for idx in v.owned:
            assert np.array_equal(s.get_b(idx), fitted[idx][0]) and s.get_f(idx).shape == fitted[idx][1].shape
