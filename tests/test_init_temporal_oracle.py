"""initTemporal on the CPU: the fixtures' margins, the float64 oracle's own properties (tests/init_temporal_oracle.py) and the host side of
Sources2D.initTemporal / set_W / set_b0 against a fake engine."""
import os
import sys

import numpy as np
import pytest
import scipy.sparse as sp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import init_temporal_cases as itc
import init_temporal_oracle as ito


def rel(a, b):
    a = np.asarray(a, dtype=np.float64); b = np.asarray(b, dtype=np.float64)
    return float(np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-300))


@pytest.mark.parametrize("name", sorted(itc.CASES))
def test_fixture_margins(name):
    """the winner of every pixel of the rough start beats the runner-up by MARGIN relative: no implementation can differ from the oracle in a discrete choice"""
    ref = itc.reference(name)
    assert ref["per_patch"]
    for key, res in ref["per_patch"].items():
        m = ito.winner_margins(res["tmpA"])
        assert m.size > 0 and m.min() >= itc.MARGIN, (name, key, m.min())


def test_case_a_geometry():
    """what case A is there to reach: four blocks, one of them without a neuron, a neuron on a patch border, T % 4 = 3"""
    c, ref = itc.make("A"), itc.reference("A")
    assert c.T % 4 == 3 and len(ref["ind"]) == 4
    assert sorted(k for k, ind in ref["ind"].items() if ind.size == 0) == [(1, 1)]
    for key in [(0, 0), (0, 1)]:
        assert 1 in ref["ind"][key] and ref["per_patch"][key]["AA"][list(ref["ind"][key]).index(1)] > 0      # neuron 1 has pixels in both patches


def test_case_d_crowds_one_block():
    """case D: more than 64 columns of (E - W)' [At, tmp_A] meet one 16 x 16 block (2 x 80 columns over the spot)"""
    c = itc.make("D")
    rows = c.A.indices % c.d1; cols = c.A.indices // c.d1
    assert c.K == 80 and np.ptp(rows) < 16 and np.ptp(cols) < 16


@pytest.mark.parametrize("name", ["A", "B", "C"])
def test_oracle_recovers_planted_traces(name):
    c = itc.make(name, 0.0)                                  # the second recording without its pixel noise
    ref = ito.init_temporal(c.Y, c.A, c.W, c.d1, c.d2, c.pdims, c.r, None)
    for k in range(c.K):
        assert np.corrcoef(ref["C_raw"][k], c.C_true[k])[0, 1] > 0.95, (name, k)


@pytest.mark.parametrize("name", ["A", "B"])
def test_oracle_shift_invariance(name):
    """the plain sweeps: projecting Y - mean(Y, 2) instead of Y changes no output, every row update ends in "minus its minimum" (HALS_temporal.m:66)"""
    c = itc.make(name)
    ref = itc.reference(name) if c.deconv is None else ito.init_temporal(c.Y, c.A, c.W, c.d1, c.d2, c.pdims, c.r, None)
    sh = ito.init_temporal(c.Y, c.A, c.W, c.d1, c.d2, c.pdims, c.r, None, shift=c.Y.astype(np.float64).mean(axis=0))
    for key in ["C_raw", "C"]:
        assert rel(sh[key], ref[key]) <= 1e-10, (key, rel(sh[key], ref[key]))
    # ... while the projections themselves do change
    p0, p1 = next(iter(ref["per_patch"].values())), next(iter(sh["per_patch"].values()))
    assert rel(p1["C0"], p0["C0"]) > 1e-6


def test_deconvolution_branch_is_not_shift_invariant():
    """HALS_temporal.m:79 takes GetSn of ck_raw BEFORE the baseline is removed (:88), and Welch's windowed periodogram leaks a constant into the band it
    averages: with deconvolution options the offset of the raw video's projection reaches sn, smin and the spikes.  An implementation that projects the
    centred video must put that constant back for these sweeps.  (Case B: (E - W) Ymean is hundreds per pixel -- the fitted W carries an intercept.)"""
    import oasis_oracle as oo
    x = np.random.default_rng(0).normal(size=600)
    assert abs(oo.GetSn(x + 1000.0) / oo.GetSn(x) - 1) > 0.1
    c, ref = itc.make("B"), itc.reference("B")
    sh = ito.init_temporal(c.Y, c.A, c.W, c.d1, c.d2, c.pdims, c.r, c.deconv, shift=c.Y.astype(np.float64).mean(axis=0))
    p0, p1 = ref["per_patch"][(0, 0)], sh["per_patch"][(0, 0)]
    assert np.all(p0["sn"] > 2 * p1["sn"]) and rel(p1["C_raw"], p0["C_raw"]) > 1e-3


def test_stitch_uses_AA_not_aa():
    """a neuron on two patches is averaged with AA = sum(A(patch, k).^2) of the ORIGINAL footprint (initTemporal.m:160,285), not with the regression's aa"""
    ref = itc.reference("A")
    k = 1
    parts = [(res, list(ref["ind"][key]).index(k)) for key, res in ref["per_patch"].items() if k in ref["ind"][key]]
    assert len(parts) == 2
    by_AA = sum(r["C_raw"][j] * r["AA"][j] for r, j in parts) / sum(r["AA"][j] for r, j in parts)
    aa = [float((r["At"][:, j] ** 2).sum()) for r, j in parts]
    by_aa = sum(r["C_raw"][j] * a for (r, j), a in zip(parts, aa)) / sum(aa)
    assert rel(ref["C_raw"][k], by_AA) <= 1e-14
    assert rel(by_aa, by_AA) > 1e-4                          # the two weightings are told apart by this fixture


def _fake_engine():
    from fake_engine import FakeEngine

    class InitFakeEngine(FakeEngine):
        supports_init_temporal = True

        def __init__(self):
            super().__init__()
            self.calls = []

        def ring_set_values(self, pid, val):
            W = self.p[pid]["W"].copy()
            W.data = np.asarray(val, dtype=np.float64).copy()
            self.p[pid]["W"] = W

        def set_b0(self, pid, b0):
            self.p[pid]["b0"] = np.asarray(b0, dtype=np.float64).copy()

        def init_temporal(self, pid, A_block, iters_plain=10, iters_last=2, deconv_options=None, want=True):
            q = self.p[pid]
            self.calls.append((pid, sp.csc_matrix(A_block).copy()))
            res = ito.init_temporal_patch(q["Y"].T, A_block, q["W"], q["ip"], None if deconv_options is None else self._dopt(deconv_options), (iters_plain, iters_last))
            self._last = (res["C_raw"], res["AA"])
            return res["C"], res["C_raw"], res["S"], res["kernel_pars"], res["sn"], res["AA"]
    return InitFakeEngine()


def _fake_sources(name, **opt):
    from cnmf_e_amd.sources2d import PatchedVideo, Sources2D, Options
    c = itc.make(name)
    eng = _fake_engine()
    video = PatchedVideo(c.d1, c.d2, c.T, c.pdims, c.r, eng)
    video.upload_from_full(c.Y.astype(np.float64))
    s = Sources2D(video, Options(ring_radius=c.r, **opt), c.A, np.zeros((c.K, c.T), np.float32), np.ones(c.d1 * c.d2, np.float32))
    for idx in video.owned:
        s.set_W(idx, c.W[idx]); s.set_b0(idx, c.b0[idx])
    return c, eng, video, s


def test_host_slicing_against_fake_engine():
    """Sources2D.initTemporal: per patch the neurons with weight in the BLOCK and their block rows, P.Ymean, the AA stitch, C = C_raw"""
    c, eng, video, s = _fake_sources("A")
    ref = itc.reference("A")
    for idx in video.owned:                                  # set_W put the fitted values on the ring pattern; the first-run test sees a fitted W
        assert rel(s.get_W(idx).toarray(), c.W[idx].toarray()) == 0 and not eng.ring_first_run(video.pid[idx])
        assert np.array_equal(s.get_b0(idx), c.b0[idx].astype(np.float64))
    out = s.initTemporal()
    assert out is s.C and s.C is s.C_raw
    called = {pid: A for pid, A in eng.calls}
    for idx in video.owned:
        ind = ref["ind"][idx]
        if ind.size == 0:
            assert video.pid[idx] not in called              # initTemporal.m:156-159
            continue
        want = sp.csc_matrix(c.A)[video.block_pix[idx]][:, ind]
        assert (called[video.pid[idx]] != want).nnz == 0
        assert np.allclose(s.P["Ymean"][idx], c.Y[:, video.patch_pix[idx]].astype(np.float64).mean(axis=0), rtol=1e-12)
    assert rel(s.C_raw, ref["C_raw"]) <= 1e-6                 # (the fake stitch hands float32 back)


def test_host_deconv_and_refusals():
    c, eng, video, s = _fake_sources("B", deconv_flag=True)
    ref = itc.reference("B")
    s.initTemporal(frame_range=(1, c.T))
    assert rel(s.C_raw, ref["C_raw"]) <= 1e-5 and rel(s.C, ref["C"]) <= 1e-5 and rel(s.S, ref["S"]) <= 1e-5
    assert np.allclose(s.P["kernel_pars"], ref["kernel_pars"], atol=1e-6) and np.allclose(s.P["neuron_sn"], ref["neuron_sn"], rtol=1e-5)
    before = (s.C, s.C_raw)
    with pytest.raises(NotImplementedError):
        s.initTemporal(frame_range=(2, c.T))
    s.ssub = 2
    with pytest.raises(NotImplementedError):
        s.initTemporal()
    s.ssub = 1
    s.A = sp.csc_matrix((c.d1 * c.d2, 0), dtype=np.float32)
    with pytest.raises(ValueError):
        s.initTemporal()
    assert s.C is before[0] and s.C_raw is before[1]          # a refused call leaves the object as it was
    with pytest.raises(ValueError):
        s.set_W(video.owned[0], np.zeros(3, np.float32))
    with pytest.raises(ValueError):
        s.set_b0(video.owned[0], np.zeros(3, np.float32))
