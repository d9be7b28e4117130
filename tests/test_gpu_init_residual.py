"""The second initialisation pass on the device: Sources2D.initComponents_residual_parallel (cnmfe_peel_open_residual + the peel session of csrc/peel.hpp on
patch geometry) against the float64 oracle (OracleSources2D.init_residual, tests/greedy_oracle.py::greedy_block) on the fixtures of tests/residual_cases.py.

1. the session's video: the exported Yres against the oracle's init_residual (the engine's W, b0 copied in), max |diff| / std(ref) <= 2e-4 -- the bound
   tests/test_gpu_parity.py::test_init_residual_parity asserts of this expression.
2. steps under forced seeds and the automatic search end to end, as tests/test_gpu_init.py does it.  The oracle's greedy run takes THE EXPORTED Yres (fp32, as
   float64) as its input: both sides start from the same numbers and the comparison isolates the session.  The discrete decisions must be EQUAL; each test first
   asserts that this oracle run's decision margins are at least half the bounds of tests/greedy_cases.py (a failure there is a fixture failure: take the next
   candidate of scripts/residual_seed_scan.py).
3. bookkeeping, 4. isolation (no trace in the fit state; two runs and two lanes bit-identical), 5. edges through the ABI.

Bounds of 2: those tests/test_gpu_init.py asserts (ci 2e-6, ai 3e-5, PNR 3e-5, Cn 6e-6, A 2e-5, C 2e-6, deconvolution 5e-6 / gamma 2e-6), kept where the error
observed on the MI355X stays below a tenth of them, else 10 x the observed error rounded up to one digit and never above 1e-4 (the rule of
tests/test_gpu_parity.py).  Observed on the MI355X (recorded per case through the `observed` fixture):
    session video, max |diff| / std(ref):  P 1.2e-4 (also with a patch that has no neuron),  S (bg_ssub 2) 7.4e-5          bound 2e-4
    steps (forced seeds)   ci / max|ci|   ai / max|ai|   PNR relative   Cn absolute
        P                  1.3e-7         5.1e-8         1.5e-6         8.5e-8
        Q                  1.3e-7         4.4e-8         8.4e-7         1.1e-7
        S                  1.6e-7         4.9e-8         7.3e-7         5.2e-8
        D                  7.8e-8         4.4e-8         6.8e-7         9.5e-8
    end to end: A / max|A| 8.1e-8 (Q), C and C_raw / max 1.7e-7 (S); case D: C 6.2e-8, C_raw 6.6e-8, S 6.7e-8 (Frobenius), gamma 2.7e-8
Every figure is below a tenth of its starting bound (ci 1.6e-7 < 2e-7, ai 5.1e-8 < 3e-6, PNR 1.5e-6 < 3e-6, Cn 1.1e-7 < 6e-7, A 8.1e-8 < 2e-6, C 1.7e-7 < 2e-7,
deconvolution 6.7e-8 < 5e-7, gamma 2.7e-8 < 2e-7): the bounds of tests/test_gpu_init.py stand unchanged."""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import residual_cases as rc
from parity_util import rel

pytestmark = pytest.mark.gpu

VIDEO_TOL = 2e-4      # max |Yres - ref| / std(ref): test_init_residual_parity's bound for this expression
CI_TOL = 2e-6         # the bounds of tests/test_gpu_init.py
AI_TOL = 3e-5
PNR_TOL = 3e-5
CN_TOL = 6e-6
A_TOL = 2e-5
C_TOL = 2e-6
DECONV_TOL = 5e-6
GAMMA_TOL = 2e-6

_runs, _oras = {}, {}


def _build(name, lanes=1, cols=None):
    """(engine, video, Sources2D) of a case after one update_background_parallel; cols: the neurons of the withholding model that are kept (default all)"""
    from cnmf_e_amd.engine import Engine
    from cnmf_e_amd.sources2d import PatchedVideo, Sources2D
    c = rc.CASES[name]
    f, Y, A0, C0 = rc.inputs(name)
    if cols is not None:
        A0, C0 = A0[:, cols], C0[cols]
    d1, d2 = c["dims"]
    eng = Engine(0)
    try:
        if lanes != 1:
            eng.set_option("lanes", lanes)
        video = PatchedVideo(d1, d2, c["T"], rc.pdims(c), c["r"], eng)
        video.upload_from_full(Y)
        s = Sources2D(video, rc.options(name), A0, C0, f.sn)
        s.update_background_parallel()
    except Exception:
        eng.close()
        raise
    return eng, video, s


def _oracle_of(name, s, video, cols=None):
    """the oracle object of the case with the engine's W, b0 (and model) copied in: the expression is what is compared"""
    o = rc.oracle_object(name)
    if cols is not None:
        o.A = o.A[:, cols]; o.C = o.C[cols]
    for idx in video.owned:
        o.W[idx] = s.get_W(idx).astype(np.float64); o.b0[idx] = np.asarray(s.get_b0(idx), dtype=np.float64)
    return o


def _run(name, seeds=None, lanes=1):
    """initComponents_residual_parallel of a case on a fresh engine -> dict(center, Cn, PNR, A / C / C_raw / S of the NEW neurons, ..., vids: the exported Yres per
    patch, opened: the opening images per patch, steps)"""
    c = rc.CASES[name]
    eng, video, s = _build(name, lanes)
    try:
        K_old = s.A.shape[1]
        A_old, C_old = s.A.toarray(), np.asarray(s.C, dtype=np.float32).copy()
        s.ids = np.arange(11, 11 + K_old); s.tags = np.zeros(K_old, dtype=np.uint16); s.P["k_ids"] = 10 + K_old
        if c.get("deconv"):
            s.S = np.zeros_like(C_old); s.P["kernel_pars"] = np.full(K_old, 0.5)
        vids, opened, log = {}, {}, {}

        def obs(idx, kind, data):
            if kind == "open":
                vids[idx] = data["Yres"]; opened[idx] = (data["Cn"], data["PNR"])
            else:
                log.setdefault(idx, []).append((kind, data))
        s._init_observer = obs
        center, Cn, PNR = s.initComponents_residual_parallel(min_corr=c["min_corr"], min_pnr=c["min_pnr"], seeds=seeds)
        A_all = s.A.toarray()
        return dict(center=center, Cn=Cn, PNR=PNR, K_old=K_old, A_old=A_old, C_old=C_old, A_all=A_all, C_all=np.asarray(s.C, dtype=np.float32).copy(),
                    A=A_all[:, K_old:].astype(np.float64), C=np.asarray(s.C, dtype=np.float64)[K_old:], C_raw=np.asarray(s.C_raw, dtype=np.float64)[K_old:],
                    S=np.asarray(s.S, dtype=np.float64), kernel_pars=s.P.get("kernel_pars"), ids=s.ids, tags=s.tags, k_ids=s.P["k_ids"],
                    opts=(s.options.min_corr, s.options.min_pnr), has_Cn=hasattr(s, "Cn"), vids=vids, opened=opened, steps=log,
                    patch_pos={idx: [int(x) for x in video.patch_pos[idx]] for idx in video.owned})
    finally:
        eng.close()


def _auto(name):
    if name not in _runs:
        _runs[name] = _run(name)
    return _runs[name]


def _ora(name, forced=False):
    """the oracle's second pass on the videos the device exported (computed once, shared)"""
    key = (name, forced)
    if key not in _oras:
        vids = _auto(name)["vids"]
        seeds = [tuple(int(x) for x in r) for r in _ora(name)["center"]] if forced else None
        _oras[key] = rc.collect(rc.CASES[name], rc.oracle_object(name), lambda idx: vids[idx].T.astype(np.float64), seeds)
    return _oras[key]


def _forced(name):
    key = (name, "forced")
    if key not in _runs:
        _runs[key] = _run(name, seeds=[tuple(int(x) for x in r) for r in _ora(name)["center"]])
    return _runs[key]


def _fixture_ok(name, forced):
    ora = _ora(name, forced)
    bad = rc.margins_clear(ora["margins"], 0.5)
    print("margins %s %s: %s" % (name, "forced" if forced else "auto", {k: "%.2e" % v for k, v in sorted(ora["margins"].items())}))
    assert not bad and ora["center"].shape[0] >= 2, ("FIXTURE: the oracle's margins on the exported video", name, bad, ora["center"].shape[0])
    return ora


def _maxrel(a, b):
    return float(np.max(np.abs(np.asarray(a) - np.asarray(b))) / np.max(np.abs(b)))


# ---- 1. the session's video ------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,cols", [("P", None), ("P", [0, 2, 3]), ("S", None)], ids=["P", "P-empty-patch", "S-bg_ssub2"])
def test_session_video_parity(name, cols, observed):
    """Yres_out against OracleSources2D.init_residual.  Case P holds a neuron (0) that lies only in the halo of patch (1, 0): its patch rows of A are empty; with
    neuron 1 dropped from the model, patch (0, 0) has no neuron at all (Ksel = 0: the session searches Ysig itself)."""
    from cnmf_e_amd.sources2d import seed_psf
    c = rc.CASES[name]
    eng, video, s = _build(name, cols=cols)
    try:
        o = _oracle_of(name, s, video, cols)
        psf = seed_psf(c["gSig"], c["gSiz"], True)
        worst, kinds = 0.0, set()
        for idx in video.owned:
            pid = video.pid[idx]
            ind, A_blk = s._slice(s.A, idx, "block")
            C_blk = s._rows(s.C, ind) if ind.size else None
            s._residual(idx, A_blk if ind.size else None, C_blk)
            A_pp = s._slice(s.A, idx, "patch", cols=ind)[1] if ind.size else None
            if A_pp is None:
                kinds.add("no neuron")
            elif np.any(np.diff(A_pp.tocsc().indptr) == 0):
                kinds.add("halo only")
            cn, pnr, sn, got = eng.peel_open_residual(pid, A_pp, C_blk, psf, want_video=True)
            eng.peel_close(pid)
            ref = o.init_residual(idx)
            assert got.shape == ref.T.shape and cn.shape == pnr.shape == sn.shape == (ref.shape[0],)
            worst = max(worst, float(np.abs(got.T.astype(np.float64) - ref).max() / ref.std()))
        observed["init_residual_video_%s%s" % (name, "" if cols is None else "_empty")] = worst
        print("session video %s: max |diff| / std = %.3e  (%s)" % (name, worst, sorted(kinds)))
        if name == "P":
            assert ("halo only" in kinds) and (cols is None or "no neuron" in kinds), kinds
        assert worst <= VIDEO_TOL, worst
    finally:
        eng.close()


# ---- 2. steps under forced seeds, the automatic search end to end -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(rc.CASES))
def test_step_parity_under_forced_seeds(name, observed):
    ora = _fixture_ok(name, True)
    got = _forced(name)
    for idx, v in _auto(name)["vids"].items():                            # two sessions are opened on the same video, bit for bit
        assert np.array_equal(v, got["vids"][idx])
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
    observed["init_residual_steps_%s" % name] = e
    print("residual init steps %s: %d steps  ci %.3e  ai %.3e  PNR rel %.3e  Cn abs %.3e" % (name, nsteps, e["ci"], e["ai"], e["pnr"], e["cn"]))
    assert nsteps >= 4
    assert np.array_equal(got["center"], ora["center"])
    assert e["ci"] <= CI_TOL and e["ai"] <= AI_TOL and e["pnr"] <= PNR_TOL and e["cn"] <= CN_TOL, e


@pytest.mark.parametrize("name", list(rc.CASES))
def test_end_to_end_automatic_search(name, observed):
    ora = _fixture_ok(name, False)
    got = _auto(name)
    c = rc.CASES[name]
    assert np.array_equal(got["center"], ora["center"]), (got["center"], ora["center"])
    K = ora["center"].shape[0]
    assert got["A"].shape == ora["A"].shape and got["C"].shape == (K, c["T"])
    e = dict(A=_maxrel(got["A"], ora["A"]), C=_maxrel(got["C"], ora["C"]), C_raw=_maxrel(got["C_raw"], ora["C_raw"]))
    S_new = got["S"][got["K_old"]:]
    if c.get("deconv"):
        e["C_fro"] = max(rel(got["C"][k], ora["C"][k]) for k in range(K))
        e["C_raw_fro"] = max(rel(got["C_raw"][k], ora["C_raw"][k]) for k in range(K))
        e["S_fro"] = max(rel(S_new[k], ora["S"][k]) for k in range(K))
        e["gamma"] = float(np.max(np.abs(np.asarray(got["kernel_pars"], dtype=np.float64)[got["K_old"]:] - np.asarray(ora["kernel_pars"], dtype=np.float64))))
    observed["init_residual_e2e_%s" % name] = e
    print("residual init e2e %s: K %d  %s" % (name, K, {k: "%.3e" % v for k, v in e.items()}))
    assert np.array_equal(got["A"] != 0, ora["A"] != 0)
    if c.get("deconv"):
        assert e["A"] <= A_TOL
        assert e["C_fro"] <= DECONV_TOL and e["C_raw_fro"] <= DECONV_TOL and e["S_fro"] <= DECONV_TOL and e["gamma"] <= GAMMA_TOL, e
    else:
        assert e["A"] <= A_TOL and e["C"] <= C_TOL and e["C_raw"] <= C_TOL, e
        assert not S_new.any()


# ---- 3. bookkeeping -----------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["P", "D"])
def test_bookkeeping(name):
    got = _auto(name)
    c = rc.CASES[name]
    K_old, K_new = got["K_old"], got["center"].shape[0]
    assert K_new >= 2 and got["A_all"].shape[1] == K_old + K_new and got["C_all"].shape == (K_old + K_new, c["T"])
    assert np.array_equal(got["A_all"][:, :K_old], got["A_old"]) and np.array_equal(got["C_all"][:K_old], got["C_old"])      # appended behind; the old part bit-unchanged
    assert np.array_equal(got["ids"], np.concatenate([np.arange(11, 11 + K_old), 10 + K_old + np.arange(1, K_new + 1)]))
    assert got["tags"].shape == (K_old + K_new,) and not got["tags"].any() and got["k_ids"] == 10 + K_old + K_new
    assert got["S"].shape == (K_old + K_new, c["T"])
    if c.get("deconv"):
        assert len(got["kernel_pars"]) == K_old + K_new and np.all(np.asarray(got["kernel_pars"])[:K_old] == 0.5)
    assert got["opts"] == (c["min_corr"], c["min_pnr"]) and not got["has_Cn"]                # the overwritten options persist; obj.Cn is not touched
    d1, d2 = c["dims"]
    assert got["Cn"].shape == got["PNR"].shape == (d1, d2) and len(got["opened"]) == len(got["patch_pos"])
    for idx, (cn, pnr) in got["opened"].items():                                             # the opening images placed by patch
        pp = got["patch_pos"][idx]
        sh = (pp[1] - pp[0] + 1, pp[3] - pp[2] + 1)
        assert np.array_equal(got["Cn"][pp[0] - 1:pp[1], pp[2] - 1:pp[3]], cn.astype(np.float64).reshape(sh, order="F"))
        assert np.array_equal(got["PNR"][pp[0] - 1:pp[1], pp[2] - 1:pp[3]], pnr.astype(np.float64).reshape(sh, order="F"))


# ---- 4. isolation ---------------------------------------------------------------------------------------------------------------------------------------------------
def _iteration_after(name, with_session, comps=None):
    eng, video, s = _build(name)
    try:
        c = rc.CASES[name]
        if with_session:
            s.initComponents_residual_parallel(min_corr=c["min_corr"], min_pnr=c["min_pnr"])
            comps = (s.A.copy(), np.asarray(s.C, dtype=np.float32).copy(), np.asarray(s.C_raw, dtype=np.float32).copy())
        else:
            s.set_components(*comps)
        s.update_spatial_parallel(update_sn=True)
        A = s.A.toarray()
        s.update_temporal_parallel()
        W = [s.get_W(idx).data.copy() for idx in video.owned]
        b0 = [np.asarray(s.get_b0(idx)).copy() for idx in video.owned]
        return comps, (A, np.asarray(s.C, dtype=np.float32).copy(), W, b0, np.asarray(s.P["sn"]).copy())
    finally:
        eng.close()


@pytest.mark.parametrize("name", ["P", "S"])
def test_the_session_leaves_no_trace_in_the_fit_state(name):
    """update_background -> the second pass -> update_spatial(update_sn) -> update_temporal against an object that was handed the same appended A, C, C_raw through
    set_components instead of running the sessions: A, C, W, b0 (and P.sn) equal bit for bit"""
    comps, (A1, C1, W1, b1, sn1) = _iteration_after(name, True)
    assert comps[0].shape[1] > rc.CASES[name]["K"] - rc.CASES[name]["hold"]
    _, (A0, C0, W0, b0, sn0) = _iteration_after(name, False, comps)
    assert np.array_equal(A0, A1) and np.array_equal(C0, C1) and np.array_equal(sn0, sn1)
    assert all(np.array_equal(a, b) for a, b in zip(W0, W1)) and all(np.array_equal(a, b) for a, b in zip(b0, b1))


def test_two_runs_and_two_lanes_are_bit_identical():
    a, b, l2 = _auto("P"), _run("P"), _run("P", lanes=2)
    for other in (b, l2):
        assert np.array_equal(a["center"], other["center"]) and np.array_equal(a["A_all"], other["A_all"]) and np.array_equal(a["C_all"], other["C_all"])
        assert np.array_equal(a["Cn"], other["Cn"]) and np.array_equal(a["PNR"], other["PNR"])


# ---- 5. edges through the ABI: return codes ----------------------------------------------------------------------------------------------------------------
def test_edges_return_codes():
    from cnmf_e_amd._lib import CnmfeError
    from cnmf_e_amd.sources2d import seed_psf
    c = rc.CASES["P"]
    psf = seed_psf(c["gSig"], c["gSiz"], True)
    g = int(c["gSiz"])
    eng, video, s = _build("P")
    try:
        idx = (0, 0)
        pid = video.pid[idx]
        pp, bp = video.patch_pos[idx], video.block_pos[idx]
        nr, nc = int(pp[1] - pp[0] + 1), int(pp[3] - pp[2] + 1)
        nr_b = int(bp[1] - bp[0] + 1)
        assert nr_b > nr                                                  # the block is larger than the patch: a seed in the halo is outside the session
        ind, A_blk = s._slice(s.A, idx, "block")
        C_blk = s._rows(s.C, ind)
        A_pp = s._slice(s.A, idx, "patch", cols=ind)[1]
        with pytest.raises(CnmfeError, match="error -4"):                 # the fit left no resident residual
            eng.peel_open_residual(pid, A_pp, C_blk, psf)
        eng.peel_open(pid, psf); eng.peel_close(pid)                      # ... and the refused call left no session behind
        s._residual(idx, A_blk, C_blk)
        sn0 = eng.get_sn(pid)
        cn, pnr, sn, _ = eng.peel_open_residual(pid, A_pp, C_blk, psf)
        assert cn.shape == (nr * nc,)
        with pytest.raises(CnmfeError, match="error -4"):                 # a second open, of either kind
            eng.peel_open_residual(pid, A_pp, C_blk, psf)
        with pytest.raises(CnmfeError, match="error -4"):
            eng.peel_open(pid, psf)
        with pytest.raises(CnmfeError, match="error -1"):                 # inside the block, outside the patch
            eng.peel_extract(pid, nr, 5, g)
        with pytest.raises(CnmfeError, match="error -5"):
            eng.peel_extract(pid, 5, 5, 21)
        r, q = nr // 2, nc // 2
        corr, ai, ci, st = eng.peel_extract(pid, r, q, g)
        r0, r1, c0, c1 = eng.peel_box(nr, nc, r, q, g)
        s0, s1, t0, t1 = eng.peel_box(nr, nc, r, q, 2 * g)
        assert corr.shape == (r1 - r0, c1 - c0) and abs(corr[r - r0, q - c0] - 1.0) < 1e-12
        big = np.zeros((s1 - s0, t1 - t0)); big[r0 - s0:r1 - s0, c0 - t0:c1 - t0] = ai
        p2, c2 = eng.peel_apply(pid, r, q, g, ai, big, np.nan_to_num(ci), 3.0, 5.0, 0.6)
        assert p2.shape == c2.shape == (s1 - s0, t1 - t0)
        assert np.array_equal(eng.get_sn(pid), sn0)                       # the peel worked on the session's copies: Ysig is what it was
        eng.peel_close(pid)
        with pytest.raises(CnmfeError, match="error -4"):                 # the residual went with the session
            eng.peel_open_residual(pid, A_pp, C_blk, psf)
        # a block session and a residual session on the same patch, one after the other, both work -- on their own geometry
        cn_b, _, _ = eng.peel_open(pid, psf)
        assert cn_b.shape == (nr_b * int(bp[3] - bp[2] + 1),)
        eng.peel_extract(pid, nr, 5, g)                                   # the same seed is inside the block
        eng.peel_close(pid)
        s._residual(idx, A_blk, C_blk)
        cn2, pnr2, sn2, _ = eng.peel_open_residual(pid, A_pp, C_blk, psf)
        eng.peel_close(pid)
        assert np.array_equal(cn, cn2) and np.array_equal(pnr, pnr2) and np.array_equal(sn, sn2)
        for kw in (dict(save_avi=True),):
            with pytest.raises(NotImplementedError):
                s.initComponents_residual_parallel(**kw)
        for bad in (dict(ssub=2), dict(tsub=2)):
            s.options = rc.options("P", **bad)
            with pytest.raises(NotImplementedError):
                s.initComponents_residual_parallel()
    finally:
        eng.close()
