"""CPU tests of the second initialisation pass (Sources2D.initComponents_residual_parallel):

1. the FIXTURE CHECK that entitles tests/test_gpu_init_residual.py to demand identical discrete decisions: for every case of tests/residual_cases.py the float64
   oracle (OracleSources2D.init_residual -> greedy_oracle.greedy_block on the patch) finds at least two neurons in the automatic search and in the forced-seed run,
   and its decision margins clear the bounds of tests/greedy_cases.py.  A case that fails here needs another synthetic seed, not another bound.
2. the method's HOST logic -- the residual request, the patch-relative seeds and margins, the stitch by patch position, the appended bookkeeping -- over a test
   double whose peel session is the oracle's arithmetic (tests/fake_engine.py + _OracleSession of tests/test_greedy_oracle.py): it must retrace the oracle's run."""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import greedy_cases as gc
import residual_cases as rc


@pytest.mark.parametrize("forced", [False, True], ids=["auto", "forced"])
@pytest.mark.parametrize("name", list(rc.CASES))
def test_fixture_margins(name, forced):
    res = rc.oracle(name, forced)
    mg = res["margins"]
    print(name, "forced" if forced else "auto", "K", res["center"].shape[0], {k: "%.2e" % v for k, v in sorted(mg.items())})
    assert res["center"].shape[0] >= 2
    if forced:
        assert np.array_equal(res["center"], rc.oracle(name)["center"])
    for key in ("corr", "cn", "pnr", "diff", "hy"):
        assert key in mg, key
    for key, val in mg.items():
        assert val >= gc.MARGIN_MIN.get(key, gc.MARGIN_DEFAULT), (name, key, val)


def test_the_withheld_neurons_are_what_the_second_pass_finds():
    """every centre the oracle accepts in case P lies within 2 pixels of the centre of mass of a neuron the model was not given"""
    c = rc.CASES["P"]
    f = rc.inputs("P")[0]
    d1, d2 = c["dims"]
    A = f.A_true.toarray()[:, c["K"] - c["hold"]:]
    rr, cc = np.arange(d1 * d2) % d1 + 1, np.arange(d1 * d2) // d1 + 1
    com = np.stack([(A * rr[:, None]).sum(0) / A.sum(0), (A * cc[:, None]).sum(0) / A.sum(0)], axis=1)
    for ctr in rc.oracle("P")["center"]:
        assert np.min(np.hypot(com[:, 0] - ctr[0], com[:, 1] - ctr[1])) <= 2.0, (ctr, com)


def _double():
    from fake_engine import FakeEngine
    from test_greedy_oracle import _OracleSession

    class ResidualDouble(FakeEngine):
        """FakeEngine + the residual peel session as the oracle computes it"""
        def peel_open_residual(self, pid, A_patch, C, psf, sig=3.0, want_video=False):
            q = self.p[pid]
            assert "Ysig" in q and "peel" not in q
            R = q["Ysig"] if A_patch is None else q["Ysig"] - np.asarray(A_patch.astype(np.float64) @ np.asarray(C, dtype=np.float64))
            nr, nc = int(q["pr"][1] - q["pr"][0] + 1), int(q["pr"][3] - q["pr"][2] + 1)
            s = q["peel"] = _OracleSession(R, nr, nc, self.gSig, self.gSiz, 1)
            return s.Cn.reshape(-1, order="F"), s.PNR.reshape(-1, order="F"), s.Sn, (R.T.copy() if want_video else None)

        def peel_open(self, pid, psf, nframes=None, Q=None, sig=3.0, frame0=0):
            q = self.p[pid]
            nr, nc = int(q["br"][1] - q["br"][0] + 1), int(q["br"][3] - q["br"][2] + 1)
            s = q["peel"] = _OracleSession(q["Y"].T, nr, nc, self.gSig, self.gSiz, 1)
            return s.Cn.reshape(-1, order="F"), s.PNR.reshape(-1, order="F"), s.Sn

        def peel_extract(self, pid, r, c, gSiz):
            return self.p[pid]["peel"].extract(r, c)

        def peel_apply(self, pid, r, c, gSiz, ai, Hai, ci, sig, min_pnr, min_corr):
            return self.p[pid]["peel"].apply(r, c, ai, Hai, ci, sig, min_pnr, min_corr)

        def peel_close(self, pid):
            del self.p[pid]["peel"]
            self.p[pid].pop("Ysig", None)                    # the residual of a residual session goes with it
    return ResidualDouble()


@pytest.mark.parametrize("name", ["P", "D"])
def test_host_method_retraces_the_oracle(name):
    from cnmf_e_amd.sources2d import PatchedVideo, Sources2D
    c = rc.CASES[name]
    f, Y, A0, C0 = rc.inputs(name)
    d1, d2 = c["dims"]
    eng = _double()
    eng.gSig, eng.gSiz = c["gSig"], c["gSiz"]
    video = PatchedVideo(d1, d2, c["T"], rc.pdims(c), c["r"], eng)
    video.upload_from_full(Y)
    s = Sources2D(video, rc.options(name), A0, C0, f.sn)
    s.update_background_parallel()
    A_old, C_old, K_old = s.A.copy(), np.asarray(s.C).copy(), A0.shape[1]
    s.ids = np.arange(11, 11 + K_old); s.tags = np.zeros(K_old, dtype=np.uint16); s.P["k_ids"] = 10 + K_old
    if c.get("deconv"):
        s.S = np.zeros_like(C_old); s.P["kernel_pars"] = np.full(K_old, 0.5)
    opened = {}
    s._init_observer = lambda idx, kind, data: opened.setdefault(idx, data) if kind == "open" else None
    center, Cn, PNR = s.initComponents_residual_parallel(min_corr=c["min_corr"], min_pnr=c["min_pnr"])
    ora = rc.oracle(name)
    K_new = ora["center"].shape[0]
    assert np.array_equal(center, ora["center"])
    assert s.A.shape == (d1 * d2, K_old + K_new) and s.C.shape == (K_old + K_new, c["T"]) and s.C_raw.shape == s.C.shape and s.S.shape == s.C.shape
    # appended behind the old columns, which are unchanged
    assert np.array_equal(s.A[:, :K_old].toarray(), A_old.toarray()) and np.array_equal(np.asarray(s.C)[:K_old], C_old)
    got_A = s.A[:, K_old:].toarray().astype(np.float64)
    assert np.array_equal(got_A != 0, ora["A"].astype(np.float32) != 0)
    assert np.allclose(got_A, ora["A"], rtol=1e-6, atol=0) and np.allclose(np.asarray(s.C)[K_old:], ora["C"], rtol=1e-5, atol=1e-5)
    assert np.allclose(np.asarray(s.C_raw)[K_old:], ora["C_raw"], rtol=1e-5, atol=1e-5)
    if c.get("deconv"):
        assert len(s.P["kernel_pars"]) == K_old + K_new and np.allclose(s.P["kernel_pars"][K_old:], ora["kernel_pars"], atol=1e-6) and s.S[K_old:].any()
    else:
        assert not s.S[K_old:].any()
    assert np.array_equal(s.ids, np.concatenate([np.arange(11, 11 + K_old), 10 + K_old + np.arange(1, K_new + 1)]))
    assert s.tags.shape == (K_old + K_new,) and s.tags.dtype == np.uint16 and s.P["k_ids"] == 10 + K_old + K_new
    assert s.options.min_corr == c["min_corr"] and s.options.min_pnr == c["min_pnr"]          # the overwritten options persist
    assert s.A_prev is not s.A and s.A_prev.shape[1] == K_old and not hasattr(s, "Cn")
    # the images are the sessions' opening images placed by patch
    for idx, data in opened.items():
        pp = [int(x) for x in video.patch_pos[idx]]
        sh = (pp[1] - pp[0] + 1, pp[3] - pp[2] + 1)
        assert np.array_equal(Cn[pp[0] - 1:pp[1], pp[2] - 1:pp[3]], np.asarray(data["Cn"], dtype=np.float64).reshape(sh, order="F"))
        assert np.array_equal(PNR[pp[0] - 1:pp[1], pp[2] - 1:pp[3]], np.asarray(data["PNR"], dtype=np.float64).reshape(sh, order="F"))
    assert len(opened) == len(video.owned)
    assert all("peel" not in q for q in eng.p.values())
    for kw in (dict(save_avi=True), dict(seed_method="manual")):
        with pytest.raises((NotImplementedError, ValueError)):
            s.initComponents_residual_parallel(**kw)
    assert s.options.seed_method == "manual"


def test_the_first_pass_still_retraces_its_oracle():
    """initComponents_parallel shares its collection with the second pass (Sources2D._stitch_init): over the same double it must find what tests/greedy_oracle.py
    finds on case A of tests/greedy_cases.py (four blocks with halo, the centres kept by patch interior)"""
    from cnmf_e_amd.sources2d import PatchedVideo, Sources2D
    c = gc.CASES["A"]
    f, Y = gc.inputs("A")
    d1, d2 = c["dims"]
    eng = _double()
    eng.gSig, eng.gSiz = c["gSig"], c["gSiz"]
    video = PatchedVideo(d1, d2, c["T"], c["pdims"], c["r"], eng)
    video.upload_from_full(Y)
    s = Sources2D(video, gc.options("A"), f.A_init, f.C_init, f.sn)
    center, Cn, PNR = s.initComponents_parallel()
    ora = gc.oracle("A")
    K = ora["center"].shape[0]
    assert K >= 1 and np.array_equal(center, ora["center"]) and s.A.shape == ora["A"].shape
    assert np.allclose(s.A.toarray(), ora["A"], rtol=1e-6, atol=0) and np.allclose(np.asarray(s.C), ora["C"], rtol=1e-5, atol=1e-5)
    assert np.array_equal(s.ids, np.arange(1, K + 1)) and s.P["k_ids"] == K and s.tags.shape == (K,) and s.S.shape == s.C.shape and s.Cn is Cn
