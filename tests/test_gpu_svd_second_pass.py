"""The second initialisation pass under background_model = 'svd' on the device: cnmfe_peel_open_lowrank (csrc/peel.hpp, k_peel_yres_lowrank) and
Sources2D.initComponents_residual_parallel on the fixtures of tests/svd_second_pass_cases.py (their margins: tests/test_svd_second_pass_host.py).

(a) the session's video after a transplanted random b, f, b0 (the recipe of tests/test_gpu_svd_bg.py::test_residual_kernel_after_set) against float64:
        exact = Yc + (ymf - b0) - b f - A C,   Yc = fl32(Y - ymf)
        |got - exact| <= 2^-23 (|Yc| + |ymf - b0| + |b f| + |A C|)            one rounding to fp32 (2^-24 |exact|), with room for the fp64 sums
(b) Sources2D.initComponents_residual_parallel end to end after one update_background_parallel.  The oracle's greedy run takes THE EXPORTED video as float64
    (the method of tests/test_gpu_init_residual.py): its margins must be at least half the fixture bounds, the discrete decisions must be EQUAL, the values stay
    within the bounds of that file (ci 2e-6, ai 3e-5, PNR 3e-5, Cn 6e-6, A 2e-5, C 2e-6, deconvolution 5e-6, gamma 2e-6): each is kept where the error observed
    on the MI355X stays below a tenth of it, else it becomes 10 x the observed error, never above 1e-4.
(c) bookkeeping, (d) isolation, (e) ssub = tsub = 2, (f) state rules.

Observed on the MI355X (recorded through the `observed` fixture): see OBSERVED below."""
import numpy as np
import pytest
import scipy.sparse as sp

import ds_oracle as dso
import residual_cases as rc
import svd_bg_cases as sc
import svd_second_pass_cases as sp2
from parity_util import rel

pytestmark = pytest.mark.gpu

CI_TOL = 2e-6         # the bounds of tests/test_gpu_init_residual.py
AI_TOL = 3e-5
PNR_TOL = 3e-5
CN_TOL = 6e-6
A_TOL = 2e-5
C_TOL = 2e-6
DECONV_TOL = 5e-6
GAMMA_TOL = 2e-6
# worst over the cases on the MI355X: steps ci 1.3e-7 (one), ai 3.4e-8 (quad), PNR 4.9e-7 (small), Cn 2.8e-8 (small); end to end A 6.2e-8 (quad), C and C_raw
# 1.2e-7 (quad); one_d (Frobenius) C 5.1e-8, C_raw 5.7e-8, S 6.7e-8, gamma 2.5e-8.  Every figure is below a tenth of its bound (ci 1.3e-7 < 2e-7, ai 3.4e-8 < 3e-6,
# PNR 4.9e-7 < 3e-6, Cn 2.8e-8 < 6e-7, A 6.2e-8 < 2e-6, C 1.2e-7 < 2e-7, deconvolution 6.7e-8 < 5e-7, gamma 2.5e-8 < 2e-7): the bounds stand unchanged.
# Session video (a): error / bound 0.496 .. 0.499 on every patch (one rounding is half the bound); (e): |Yds - ds(Yres)| / max|Yres| 2.3e-8 against 2.4e-7.
OBSERVED = dict(ci=1.3e-7, ai=3.4e-8, pnr=4.9e-7, cn=2.8e-8, A=6.2e-8, C=1.2e-7, C_raw=1.2e-7, deconv=6.7e-8, gamma=2.5e-8, video_over_bound=0.499, ds_video=2.3e-8)

_runs, _oras = {}, {}


def _psf():
    from cnmf_e_amd.sources2d import seed_psf
    return seed_psf(sp2.GSIG, float(sp2.GSIZ), True)


def _build(name, fit=True, **opts):
    """(engine, video, Sources2D) of a case, after one update_background_parallel unless fit=False"""
    from cnmf_e_amd.engine import Engine
    from cnmf_e_amd.sources2d import PatchedVideo, Sources2D
    c = sp2.case(name)
    rec, A0, C0 = sp2.inputs(name)
    d1, d2 = c["dims"]
    eng = Engine(0)
    try:
        video = PatchedVideo(d1, d2, c["T"], c["patch"], c["halo"], eng)
        video.upload_from_full(rec["Y"])
        s = Sources2D(video, sp2.options(name, **opts), A0, C0, np.ones(d1 * d2, np.float32))
        if fit:
            s.update_background_parallel()
    except Exception:
        eng.close()
        raise
    return eng, video, s


def _run(name):
    c = sp2.case(name)
    eng, video, s = _build(name)
    try:
        K_old = s.A.shape[1]
        A_old, C_old = s.A.toarray(), np.asarray(s.C, dtype=np.float32).copy()
        s.ids = np.arange(11, 11 + K_old); s.tags = np.zeros(K_old, dtype=np.uint16); s.P["k_ids"] = 10 + K_old
        if c.get("deconv"):
            s.S = np.zeros_like(C_old); s.P["kernel_pars"] = np.full(K_old, 0.5)
        vids, log = {}, {}

        def obs(idx, kind, data):
            if kind == "open":
                vids[idx] = data["Yres"]
            else:
                log.setdefault(idx, []).append((kind, data))
        s._init_observer = obs
        center, Cn, PNR = s.initComponents_residual_parallel(min_corr=c["min_corr"], min_pnr=c["min_pnr"])
        A_all = s.A.toarray()
        return dict(center=center, Cn=Cn, PNR=PNR, K_old=K_old, A_old=A_old, C_old=C_old, A_all=A_all, C_all=np.asarray(s.C, dtype=np.float32).copy(),
                    A=A_all[:, K_old:].astype(np.float64), C=np.asarray(s.C, dtype=np.float64)[K_old:], C_raw=np.asarray(s.C_raw, dtype=np.float64)[K_old:],
                    S=np.asarray(s.S, dtype=np.float64), kernel_pars=s.P.get("kernel_pars"), ids=s.ids, tags=s.tags, k_ids=s.P["k_ids"], vids=vids, steps=log)
    finally:
        eng.close()


def _auto(name):
    if name not in _runs:
        _runs[name] = _run(name)
    return _runs[name]


def _ora(name):
    """the oracle's second pass on the videos the device exported (computed once, shared)"""
    if name not in _oras:
        vids = _auto(name)["vids"]
        _oras[name] = sp2.collect(name, lambda idx: vids[idx].T.astype(np.float64))
    return _oras[name]


def _maxrel(a, b):
    return float(np.max(np.abs(np.asarray(a) - np.asarray(b))) / np.max(np.abs(b)))


# ---- (a) the session's video ---------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["one", "quad"])
@pytest.mark.parametrize("nb", [0, 3])
def test_session_video_is_one_rounding_of_the_exact_value(name, nb):
    from cnmf_e_amd.engine import Engine
    from cnmf_e_amd.sources2d import PatchedVideo
    case = sc.make_case(name, 1)
    eng = Engine(0)
    try:
        v = PatchedVideo(case["d1"], case["d2"], case["T"], case["patch"], case["halo"], eng)
        v.upload_from_full(case["Y"])
        rng = np.random.default_rng(7)
        A = case["A"].tocsr()
        kinds = set()
        for idx in v.order:
            pid, pp = v.pid[idx], v.patch_pix[idx]
            d = pp.size
            b = rng.normal(0.0, 20.0, (d, nb)); f = rng.normal(0.0, 1.0, (nb, case["T"])); b0 = case["Y"][:, pp].mean(axis=0, dtype=np.float64) + rng.normal(0.0, 3.0, d)
            eng.bg_svd_set(pid, b, f, b0)
            A_p = A[pp].tocsc()
            ind = np.nonzero(np.diff(A_p.indptr) > 0)[0]
            A_p, C_p = (A_p[:, ind].astype(np.float32), np.ascontiguousarray(case["C"][ind])) if ind.size else (None, None)
            kinds.add("neurons" if ind.size else "no neuron")
            cn, pnr, sn, got = eng.peel_open_lowrank(pid, 1, 1, A_p, C_p, _psf(), want_video=True)
            eng.peel_close(pid)
            assert got.shape == (case["T"], d) and got.dtype == np.float32 and cn.shape == pnr.shape == sn.shape == (d,)
            cn2, pnr2, sn2, again = eng.peel_open_lowrank(pid, 1, 1, A_p, C_p, _psf(), want_video=True)
            eng.peel_close(pid)
            assert np.array_equal(got, again) and np.array_equal(cn, cn2) and np.array_equal(pnr, pnr2) and np.array_equal(sn, sn2)      # two opens, equal bits
            got = got.T.astype(np.float64)
            ymf = eng.ymean(pid)[v.ind_patch[idx]].astype(np.float32)
            Yc = (case["Y"][:, pp] - ymf[None, :]).T.astype(np.float64)                               # fp32 subtraction, as k_center4
            dl = ymf.astype(np.float64) - b0
            AC = (A_p.astype(np.float64) @ C_p.astype(np.float64)) if ind.size else np.zeros_like(Yc)
            AC = np.asarray(AC)
            exact = Yc + dl[:, None] - b @ f - AC
            bound = 2.0 ** -23 * (np.abs(Yc) + np.abs(dl)[:, None] + np.abs(b @ f) + np.abs(AC))
            err = np.abs(got - exact)
            worst = float((err / np.maximum(bound, 1e-300)).max())
            print("peel_yres_lowrank %s nb %d patch %s (%d neurons): max error / bound %.3f" % (name, nb, idx, ind.size, worst))
            assert np.all(err <= bound), (name, idx, worst)
            assert np.all(err[:, -3:] <= bound[:, -3:]) and np.all(err[-1] <= bound[-1])                # the last three frames, the last pixel
        assert kinds == ({"neurons", "no neuron"} if name == "quad" else {"neurons"}), kinds
    finally:
        eng.close()


# ---- (b) end to end -------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(sp2.CASES))
def test_end_to_end_against_the_oracle_on_the_exported_video(name, observed):
    got = _auto(name)
    ora = _ora(name)
    c = sp2.case(name)
    bad = rc.margins_clear(ora["margins"], 0.5)
    print("margins %s: %s" % (name, {k: "%.2e" % v for k, v in sorted(ora["margins"].items())}))
    assert not bad and ora["center"].shape[0] == len(c["withheld"]), ("FIXTURE: the oracle's margins on the exported video", name, bad, ora["center"])
    # the steps of the automatic search
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
    assert nsteps >= 2
    assert np.array_equal(got["center"], ora["center"]), (got["center"], ora["center"])
    K = ora["center"].shape[0]
    assert got["A"].shape == ora["A"].shape and got["C"].shape == (K, c["T"])
    e.update(A=_maxrel(got["A"], ora["A"]), C=_maxrel(got["C"], ora["C"]), C_raw=_maxrel(got["C_raw"], ora["C_raw"]))
    S_new = got["S"][got["K_old"]:]
    if c.get("deconv"):
        e["C_fro"] = max(rel(got["C"][k], ora["C"][k]) for k in range(K))
        e["C_raw_fro"] = max(rel(got["C_raw"][k], ora["C_raw"][k]) for k in range(K))
        e["S_fro"] = max(rel(S_new[k], ora["S"][k]) for k in range(K))
        e["gamma"] = float(np.max(np.abs(np.asarray(got["kernel_pars"], dtype=np.float64)[got["K_old"]:] - np.asarray(ora["kernel_pars"], dtype=np.float64))))
    observed["svd_second_pass_%s" % name] = e
    print("svd second pass %s: K %d steps %d  %s" % (name, K, nsteps, {k: "%.3e" % v for k, v in e.items()}))
    assert e["ci"] <= CI_TOL and e["ai"] <= AI_TOL and e["pnr"] <= PNR_TOL and e["cn"] <= CN_TOL, e
    assert np.array_equal(got["A"] != 0, ora["A"] != 0)
    assert e["A"] <= A_TOL
    if c.get("deconv"):
        assert e["C_fro"] <= DECONV_TOL and e["C_raw_fro"] <= DECONV_TOL and e["S_fro"] <= DECONV_TOL and e["gamma"] <= GAMMA_TOL, e
    else:
        assert e["C"] <= C_TOL and e["C_raw"] <= C_TOL, e
        assert not S_new.any()


# ---- (c) bookkeeping --------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["one", "one_d"])
def test_bookkeeping(name):
    got = _auto(name)
    c = sp2.case(name)
    K_old, K_new = got["K_old"], got["center"].shape[0]
    assert K_new == len(c["withheld"]) and got["A_all"].shape[1] == K_old + K_new and got["C_all"].shape == (K_old + K_new, c["T"])
    assert np.array_equal(got["A_all"][:, :K_old], got["A_old"]) and np.array_equal(got["C_all"][:K_old], got["C_old"])      # appended behind; the old part bit-unchanged
    assert np.array_equal(got["ids"], np.concatenate([np.arange(11, 11 + K_old), 10 + K_old + np.arange(1, K_new + 1)]))
    assert got["tags"].shape == (K_old + K_new,) and not got["tags"].any() and got["k_ids"] == 10 + K_old + K_new
    assert got["S"].shape == (K_old + K_new, c["T"])
    if c.get("deconv"):
        assert len(got["kernel_pars"]) == K_old + K_new and np.all(np.asarray(got["kernel_pars"])[:K_old] == 0.5)
        assert got["S"][K_old:].any() and np.all(np.asarray(got["kernel_pars"])[K_old:] > 0)
    d1, d2 = c["dims"]
    assert got["Cn"].shape == got["PNR"].shape == (d1, d2)


# ---- (d) isolation ------------------------------------------------------------------------------------------------------------------------------------------------------
def _iteration_after(name, with_session, comps=None):
    eng, video, s = _build(name)
    try:
        c = sp2.case(name)
        if with_session:
            s.initComponents_residual_parallel(min_corr=c["min_corr"], min_pnr=c["min_pnr"])
            comps = (s.A.copy(), np.asarray(s.C, dtype=np.float32).copy(), np.asarray(s.C_raw, dtype=np.float32).copy())
        else:
            s.set_components(*comps)
        s.update_spatial_parallel()
        A = s.A.toarray()
        s.update_temporal_parallel()
        bg = [eng.bg_svd_get(video.pid[idx]) for idx in video.owned]
        return comps, (A, np.asarray(s.C, dtype=np.float32).copy(), bg)
    finally:
        eng.close()


@pytest.mark.parametrize("name", ["one", "quad"])
def test_the_session_leaves_no_trace_in_the_engine(name):
    """update_background -> the second pass -> update_spatial -> update_temporal against a twin that was handed the same appended A, C, C_raw through set_components
    and never ran the pass: A, C and the factors equal bit for bit"""
    comps, (A1, C1, bg1) = _iteration_after(name, True)
    assert comps[0].shape[1] > len(sp2.CASES[name]["keep"])
    _, (A0, C0, bg0) = _iteration_after(name, False, comps)
    assert np.array_equal(A0, A1) and np.array_equal(C0, C1)
    assert all(np.array_equal(x, y) for p, q in zip(bg0, bg1) for x, y in zip(p, q))


def test_two_runs_are_bit_identical():
    a, b = _auto("quad"), _run("quad")
    assert np.array_equal(a["center"], b["center"]) and np.array_equal(a["A_all"], b["A_all"]) and np.array_equal(a["C_all"], b["C_all"])
    assert np.array_equal(a["Cn"], b["Cn"]) and np.array_equal(a["PNR"], b["PNR"])
    assert all(np.array_equal(a["vids"][k], b["vids"][k]) for k in a["vids"])


def test_a_resident_residual_survives_the_session():
    """the low-rank Ysig does not depend on A or C: valid before the open, it is valid after the close, and the update gives the bits it gave"""
    eng, video, s = _build("one")
    try:
        idx = video.order[0]; pid = video.pid[idx]
        ind, A_pp = s._slice(s.A, idx, "patch")
        C_p = np.ascontiguousarray(np.asarray(s.C)[ind])
        eng.residual_lowrank(pid)
        before = eng.hals_temporal(pid, A_pp, C_p, 2)[1]
        eng.peel_open_lowrank(pid, 1, 1, A_pp, C_p, _psf())
        corr, ai, ci, st = eng.peel_extract(pid, 20, 17, sp2.GSIZ)
        eng.peel_close(pid)
        assert np.array_equal(before, eng.hals_temporal(pid, A_pp, C_p, 2)[1])                       # (no residual_lowrank in between)
    finally:
        eng.close()


# ---- (e) down-sampling ----------------------------------------------------------------------------------------------------------------------------------------------------
def test_down_sampled_session_video():
    """ssub = tsub = 2 on `one`: the opening video against dsData (tests/ds_oracle.py) of the float64 Yres, within the bound tests/test_gpu_init_residual_ds.py
    asserts of that expression: 2 * 2^-23 * max|Yres| (one rounding of the full-resolution video the device brings down, one of the output)"""
    eng, video, s = _build("one", ssub=2, tsub=2)
    try:
        c = sp2.case("one")
        rec = sp2.inputs("one")[0]
        vids = {}
        s._init_observer = lambda idx, kind, data: vids.__setitem__(idx, data["Yds"]) if kind == "open" else None
        K_old = s.A.shape[1]
        s.initComponents_residual_parallel(min_corr=c["min_corr"], min_pnr=c["min_pnr"])
        assert s.A.shape[1] >= K_old and s.C.shape[0] == s.A.shape[1]
        idx = video.order[0]; pid, pp = video.pid[idx], video.patch_pix[idx]
        nr, nc = c["dims"]
        b, f, b0 = eng.bg_svd_get(pid)
        ymf = eng.ymean(pid)[video.ind_patch[idx]].astype(np.float32)
        Yc = (rec["Y"][:, pp] - ymf[None, :]).T.astype(np.float64)
        A0, C0 = sp2.inputs("one")[1:]
        yres = Yc + (ymf.astype(np.float64) - b0)[:, None] - b @ f - np.asarray(A0.astype(np.float64) @ C0.astype(np.float64))
        want = dso.ds_block(yres, nr, nc, 2, 2)[0]
        d1s, d2s, Ts = dso.ds_dims(nr, nc, c["T"], 2, 2)
        yds = vids[idx]
        assert yds.shape == (Ts, d1s * d2s) and yds.dtype == np.float32
        e = float(np.abs(yds.T.astype(np.float64) - want).max() / np.abs(yres).max())
        print("down-sampled session video: |Yds - ds(Yres)| / max|Yres| = %.3e (bound %.3e)" % (e, 2 * 2.0 ** -23))
        assert e <= 2 * 2.0 ** -23, e
        s.update_spatial_parallel(); s.update_temporal_parallel()                                    # the dropped residual is requested again by the updates
    finally:
        eng.close()


# ---- (f) state ----------------------------------------------------------------------------------------------------------------------------------------------------------
def test_state_rules_and_seeds_outside_the_patch():
    from cnmf_e_amd._lib import CnmfeError
    from cnmf_e_amd.engine import Engine
    from cnmf_e_amd.sources2d import PatchedVideo
    c = sp2.case("small")
    rec, A0, C0 = sp2.inputs("small")
    d1, d2 = c["dims"]
    eng = Engine(0)
    try:
        video = PatchedVideo(d1, d2, c["T"], c["patch"], c["halo"], eng)
        video.upload_from_full(rec["Y"])
        pid = video.pid[video.order[0]]
        with pytest.raises(CnmfeError, match="error -4"):                     # no background yet
            eng.peel_open_lowrank(pid, 1, 1, A0, C0, _psf())
        eng.peel_open(pid, _psf()); eng.peel_close(pid)                       # ... and the refused call left no session behind
        eng.bg_svd_set(pid, np.zeros((d1 * d2, 1)), np.zeros((1, c["T"])), np.zeros(d1 * d2))
        with pytest.raises(CnmfeError, match="error -4"):                     # ... and no residual: the updates still ask for one
            eng.fast_temporal(pid, A0)
        cn, pnr, sn, y = eng.peel_open_lowrank(pid, 1, 1, A0, C0, _psf(), want_video=True)
        with pytest.raises(CnmfeError, match="error -4"):                     # a second open, of any kind
            eng.peel_open_lowrank(pid, 1, 1, A0, C0, _psf())
        with pytest.raises(CnmfeError, match="error -4"):
            eng.peel_open(pid, _psf())
        eng.peel_close(pid)
        with pytest.raises(CnmfeError, match="error -4"):                     # the session made no residual either
            eng.fast_temporal(pid, A0)
        with pytest.raises(CnmfeError, match="error -1"):
            eng.peel_open_lowrank(pid, 0, 1, A0, C0, _psf())
        with pytest.raises(CnmfeError, match="error -5"):                     # floor(301 / 5) < 64
            eng.peel_open_lowrank(pid, 1, 5, A0, C0, _psf())
        # b = f = b0 = 0: Yres = Y - A C, rounded once
        ymf = eng.ymean(pid).astype(np.float32)
        Yc = (rec["Y"] - ymf[None, :]).T.astype(np.float64)
        AC = np.asarray(A0.astype(np.float64) @ C0.astype(np.float64))
        exact = Yc + ymf.astype(np.float64)[:, None] - AC
        assert np.all(np.abs(y.T.astype(np.float64) - exact) <= 2.0 ** -23 * (np.abs(Yc) + np.abs(ymf)[:, None] + np.abs(AC)))
    finally:
        eng.close()
    eng, video, s = _build("small", fit=False)                                # no first-run refusal: the constructor's zeros are a background
    try:
        K_old = s.A.shape[1]
        center, _, _ = s.initComponents_residual_parallel(min_corr=c["min_corr"], min_pnr=c["min_pnr"], seeds=[(d1 + 5, 3), (0, 0)])
        assert center.shape[0] == 0 and s.A.shape[1] == K_old                 # seeds outside every patch are ignored
        with pytest.raises(NotImplementedError):
            s.initComponents_residual_parallel(save_avi=True)
    finally:
        eng.close()
