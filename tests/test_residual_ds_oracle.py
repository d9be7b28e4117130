"""CPU tests of the DOWN-SAMPLED second pass (options.ssub / options.tsub in Sources2D.initComponents_residual_parallel):

1. the FIXTURE CHECK that entitles tests/test_gpu_init_residual_ds.py to demand identical discrete decisions: for every case of tests/residual_ds_cases.py the
   float64 oracle (OracleSources2D.init_residual -> ds_oracle.greedy_block_ds on the patch) finds at least two neurons in the automatic search and in the
   forced-seed run, and its decision margins clear the bounds of tests/greedy_cases.py.  A case that fails here needs another synthetic seed, not another bound.
2. the LINEAR SPLIT the device relies on, in float64: ds_block(Y - A C) against ds_block(Y) - A_ds C_ds with A_ds and C_ds formed by the host code of the engine
   path (cnmf_e_amd/csrc/ds_fold.hpp through tests/ds_fold_driver.cpp, built with the host compiler and the sanitizers): the tap tables and the bin rule are
   pinned without a GPU.
3. the method's HOST logic -- the scaled parameters, the low-resolution seeds and margins, the up-sampling, the stitch by patch position, the appended
   bookkeeping -- over a test double whose peel session is the oracle's arithmetic on ds_oracle's down-sampled video: it must retrace the oracle's run.
4. the refusals: an engine without supports_init_residual_ds, factors swapped in after construction, a tsub that leaves fewer than 64 frames, factors other than 1 before any background was fitted."""
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import ds_oracle as dso
import greedy_cases as gc
import residual_ds_cases as dc


@pytest.mark.parametrize("forced", [False, True], ids=["auto", "forced"])
@pytest.mark.parametrize("name", list(dc.CASES))
def test_fixture_margins(name, forced):
    res = dc.oracle(name, forced)
    mg = res["margins"]
    print(name, "forced" if forced else "auto", "K", res["center"].shape[0], {k: "%.2e" % v for k, v in sorted(mg.items())})
    assert res["center"].shape[0] >= 2
    if forced:
        assert np.array_equal(res["center"], dc.oracle(name)["center"])
    for key in ("corr", "cn", "pnr", "diff", "hy"):
        assert key in mg, key
    for key, val in mg.items():
        assert val >= gc.MARGIN_MIN.get(key, gc.MARGIN_DEFAULT), (name, key, val)


# ---- 2. the linear split ------------------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def fold(tmp_path_factory):
    """(nr, nc, ssub, tsub, A csc float32 (nr nc x K), C float32 (K x T)) -> (A_ds dense float64 (d1s d2s x K), C_ds (K x Ts)) by ds_fold.hpp"""
    import scipy.sparse as sp
    cxx = shutil.which("g++") or shutil.which("c++")
    if cxx is None:
        pytest.skip("no host C++ compiler")
    tmp = tmp_path_factory.mktemp("ds_fold")
    exe = str(tmp / "ds_fold_driver")
    out = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-Wall", "-Wextra", "-Werror",
                          "-Wno-unused-function", os.path.join(HERE, "ds_fold_driver.cpp"), "-o", exe], capture_output=True, text=True)
    assert out.returncode == 0, out.stderr[-3000:]

    def run(nr, nc, ssub, tsub, A, C):
        A = sp.csc_matrix(A, dtype=np.float32); A.sort_indices()
        C = np.ascontiguousarray(C, dtype=np.float32)
        K, T = C.shape
        assert A.shape == (nr * nc, K)
        fin, fout = exe + ".in", exe + ".out"
        with open(fin, "wb") as fh:
            np.array([nr, nc, ssub, tsub, K, T], dtype=np.int32).tofile(fh)
            A.indptr.astype(np.int64).tofile(fh); A.indices.astype(np.int32).tofile(fh); A.data.astype(np.float32).tofile(fh); C.tofile(fh)
        r = subprocess.run([exe, fin, fout], capture_output=True, text=True)
        assert r.returncode == 0, (r.returncode, r.stderr[-3000:])
        with open(fout, "rb") as fh:
            d1s, d2s, Ts, nnz = (int(x) for x in np.fromfile(fh, dtype=np.int32, count=4))
            rowptr = np.fromfile(fh, dtype=np.int32, count=d1s * d2s + 1); col = np.fromfile(fh, dtype=np.int32, count=nnz)
            val = np.fromfile(fh, dtype=np.float64, count=nnz); cds = np.fromfile(fh, dtype=np.float64, count=K * Ts).reshape(K, Ts)
        assert (d1s, d2s, Ts) == dso.ds_dims(nr, nc, T, ssub, tsub)
        return sp.csr_matrix((val, col, rowptr), shape=(d1s * d2s, K)), cds
    return run


@pytest.mark.parametrize("name", list(dc.CASES))
def test_linear_split_in_float64(name, fold):
    """dsData(Y - A C) = dsData(Y) - A_ds C_ds on every patch of the case: Y the patch video, A the model's footprints on the patch rows (fp32, as the engine
    takes them), C their traces.  <= 1e-12 max|.|"""
    from fake_engine import FakeEngine
    from cnmf_e_amd.sources2d import PatchedVideo
    c = dc.CASES[name]
    f, Y, A0, C0 = dc.inputs(name)
    d1, d2 = c["dims"]
    video = PatchedVideo(d1, d2, c["T"], dc.pdims(c), c["r"], FakeEngine())
    hit = 0
    for idx in video.order:
        pp = [int(x) for x in video.patch_pos[idx]]
        nr, nc = pp[1] - pp[0] + 1, pp[3] - pp[2] + 1
        pix = np.asarray(video.patch_pix[idx])
        Yp = np.asarray(Y[:, pix], dtype=np.float64).T
        A_pp = A0.tocsr()[pix].tocsc().astype(np.float32)
        C = np.asarray(C0, dtype=np.float32)
        A_ds, C_ds = fold(nr, nc, c["ssub"], c["tsub"], A_pp, C)
        ref = dso.ds_block(Yp - A_pp.astype(np.float64) @ C.astype(np.float64), nr, nc, c["ssub"], c["tsub"])[0]
        got = dso.ds_block(Yp, nr, nc, c["ssub"], c["tsub"])[0] - A_ds @ C_ds
        err = float(np.abs(got - ref).max())
        print(name, idx, "nnz %d -> %d" % (A_pp.nnz, A_ds.nnz), "split error %.2e of %.2e" % (err, np.abs(ref).max()))
        assert err <= 1e-12 * max(np.abs(Yp).max(), np.abs(ref).max())
        hit += A_ds.nnz > 0
        # the bin rule and the footprint resize each on its own
        Ts = c["T"] // c["tsub"]
        assert np.abs(C_ds - C[:, :Ts * c["tsub"]].astype(np.float64).reshape(-1, Ts, c["tsub"]).mean(axis=2)).max() <= 1e-12 * max(np.abs(C).max(), 1.0)
        dense = A_pp.toarray().astype(np.float64)
        if dense.shape[1]:
            low = np.stack([dso.imresize(dense[:, k].reshape(nr, nc, order="F"), (-(-nr // c["ssub"]), -(-nc // c["ssub"])), "box").reshape(-1, order="F")
                            if c["ssub"] > 1 else dense[:, k] for k in range(dense.shape[1])], axis=1)
            assert np.abs(A_ds.toarray() - low).max() <= 1e-12 * np.abs(dense).max()
    assert hit >= 1


def test_fold_drops_zeros_and_takes_an_empty_model(fold):
    import scipy.sparse as sp
    A = sp.csc_matrix((np.array([1.0, -1.0, 2.0], dtype=np.float32), (np.array([0, 1, 22]), np.array([0, 0, 2]))), shape=(35, 3))      # column 0 cancels in its cell
    A_ds, C_ds = fold(7, 5, 2, 4, A, np.arange(3 * 70, dtype=np.float32).reshape(3, 70))
    assert A_ds.shape == (4 * 3, 3) and C_ds.shape == (3, 17)
    assert A_ds[:, 0].nnz == 0 and A_ds[:, 1].nnz == 0 and A_ds[:, 2].nnz >= 1
    assert abs(A_ds.sum() - 2.0 * dso.resize_weights(7, 4, "box")[:, 1].sum() * dso.resize_weights(5, 3, "box")[:, 3].sum()) <= 1e-14
    assert C_ds[1, 2] == np.arange(70 + 8, 70 + 12).mean()


# ---- 3. the host path over the oracle's arithmetic ---------------------------------------------------------------------------------------------------------------
def _double():
    from test_residual_oracle import _double as base
    from test_greedy_oracle import _OracleSession
    import seed_oracle as so
    cls = type(base())

    class ResidualDsDouble(cls):
        """ResidualDouble + the down-sampled residual session as ds_oracle computes it: dsData of the float64 patch residual, the oracle's session on it with the
        scaled filter"""
        supports_init_ds = True
        supports_init_residual_ds = True

        def peel_open_residual_ds(self, pid, ssub, tsub, A_patch, C, psf, sig=3.0, want_video=False):
            q = self.p[pid]
            assert "Ysig" in q and "peel" not in q
            R = q["Ysig"] if A_patch is None else q["Ysig"] - np.asarray(A_patch.astype(np.float64) @ np.asarray(C, dtype=np.float64))
            nr, nc = int(q["pr"][1] - q["pr"][0] + 1), int(q["pr"][3] - q["pr"][2] + 1)
            Yds, d1s, d2s = dso.ds_block(R, nr, nc, ssub, tsub)
            s = q["peel"] = _OracleSession(Yds, d1s, d2s, self.gSig / ssub, so.matlab_round(self.gSiz / ssub), 1)
            self.opened.append((pid, ssub, tsub, np.array(psf), (d1s, d2s), Yds.shape[1]))
            return s.Cn.reshape(-1, order="F"), s.PNR.reshape(-1, order="F"), s.Sn, (Yds.T.copy() if want_video else None)
    e = ResidualDsDouble()
    e.opened = []
    return e


def _host_run(name, seeds=None, options=None):
    from cnmf_e_amd.sources2d import PatchedVideo, Sources2D
    c = dc.CASES[name]
    f, Y, A0, C0 = dc.inputs(name)
    d1, d2 = c["dims"]
    eng = _double()
    eng.gSig, eng.gSiz = c["gSig"], c["gSiz"]
    video = PatchedVideo(d1, d2, c["T"], dc.pdims(c), c["r"], eng)
    video.upload_from_full(Y)
    s = Sources2D(video, options or dc.options(name), A0, C0, f.sn)
    s.update_background_parallel()
    return eng, video, s, A0


@pytest.mark.parametrize("name", ["A", "B", "D", "E", "F"])
def test_host_method_retraces_the_oracle(name):
    from cnmf_e_amd import hostops
    from cnmf_e_amd.sources2d import seed_psf
    c = dc.CASES[name]
    d1, d2 = c["dims"]
    ssub, tsub, T = c["ssub"], c["tsub"], c["T"]
    eng, video, s, A0 = _host_run(name)
    A_old, C_old, K_old = s.A.copy(), np.asarray(s.C).copy(), A0.shape[1]
    s.ids = np.arange(11, 11 + K_old); s.tags = np.zeros(K_old, dtype=np.uint16); s.P["k_ids"] = 10 + K_old
    if c.get("deconv"):
        s.S = np.zeros_like(C_old); s.P["kernel_pars"] = np.full(K_old, 0.5)
    opened, bds, raw = {}, {}, {}
    s._init_observer = lambda idx, kind, data: opened.setdefault(idx, data) if kind == "open" else None
    inner_block = hostops.greedy_roi_block

    def spy_block(sess, cn, pnr, gSiz, psf, min_corr, min_pnr, min_pixel, bd4, *a, **kw):
        bds[len(bds)] = (gSiz, min_pixel, list(bd4), cn.shape)
        return inner_block(sess, cn, pnr, gSiz, psf, min_corr, min_pnr, min_pixel, bd4, *a, **kw)
    inner_stitch = s._stitch_init

    def spy_stitch(per_patch, n):
        raw.update(per_patch)                                              # the float64 results before they are stored as float32
        return inner_stitch(per_patch, n)
    s._stitch_init = spy_stitch
    hostops.greedy_roi_block = spy_block
    try:
        center, Cn, PNR = s.initComponents_residual_parallel(K=c.get("Kmax"), min_corr=c["min_corr"], min_pnr=c["min_pnr"])
    finally:
        hostops.greedy_roi_block = inner_block
    ora = dc.oracle(name)
    K_new = ora["center"].shape[0]
    assert K_new >= 2 and np.array_equal(center, ora["center"])
    # the float64 results of every patch against the oracle's block: 1e-12
    import seed_oracle as so
    gz = so.matlab_round(c["gSiz"] / ssub)
    n_seen = 0
    for i, idx in enumerate(video.order):
        res, keep, org = raw[idx]
        blk = ora["blocks"][idx]
        pp = [int(x) for x in video.patch_pos[idx]]
        nr, nc = pp[1] - pp[0] + 1, pp[3] - pp[2] + 1
        edge = (idx[0] == 0, idx[0] == video.nr_patch - 1, idx[1] == 0, idx[1] == video.nc_patch - 1)
        assert org == (pp[0], pp[2])
        assert bds[i] == (gz, 5.0 / ssub ** 2, [so.matlab_round(dc.BD * int(e) / ssub) for e in edge], (-(-nr // ssub), -(-nc // ssub)))      # the scaled parameters, bd per patch
        assert np.array_equal(res["center"], blk["center"])
        for k in range(blk["center"].shape[0]):
            (r0, r1, c0, c1), ai = res["A"][k]
            img = np.zeros((nr, nc)); img[r0:r1, c0:c1] = ai
            for got, ref in ((img, blk["A"][k]), (res["C"][k], blk["C"][k]), (res["C_raw"][k], blk["C_raw"][k])):
                assert np.shape(got) == np.shape(ref) and np.abs(np.asarray(got) - ref).max() <= 1e-12 * max(np.abs(ref).max(), 1.0)
            assert len(res["C"][k]) == T
            if c.get("deconv"):
                assert np.abs(np.asarray(res["S"][k]) - blk["S"][k]).max() <= 1e-12 * max(np.abs(blk["S"][k]).max(), 1.0)
                assert abs(res["kernel_pars"][k] - blk["kernel_pars"][k]) <= 1e-12           # as fitted at the low rate
            n_seen += 1
        if ssub != 1 and blk["center"].shape[0]:
            assert np.array_equal(blk["center"], blk["low"]["center"] * ssub - 1)
    assert n_seen >= K_new
    # what the object holds (float32): appended behind the old columns, rows of length T
    assert s.A.shape == (d1 * d2, K_old + K_new) and s.C.shape == (K_old + K_new, T) and s.C_raw.shape == s.C.shape and s.S.shape == s.C.shape
    assert np.array_equal(s.A[:, :K_old].toarray(), A_old.toarray()) and np.array_equal(np.asarray(s.C)[:K_old], C_old)
    got_A = s.A[:, K_old:].toarray().astype(np.float64)
    if ssub == 1:
        assert np.array_equal(got_A != 0, ora["A"].astype(np.float32) != 0)
    assert np.allclose(got_A, ora["A"], rtol=1e-6, atol=0) and np.allclose(np.asarray(s.C)[K_old:], ora["C"], rtol=1e-5, atol=1e-5)
    assert np.allclose(np.asarray(s.C_raw)[K_old:], ora["C_raw"], rtol=1e-5, atol=1e-5)
    if ssub != 1:
        assert (got_A < 0).any()                                           # the negative lobes of the bicubic kernel are kept
    if c.get("deconv"):
        assert len(s.P["kernel_pars"]) == K_old + K_new and np.allclose(s.P["kernel_pars"][K_old:], ora["kernel_pars"], atol=1e-6) and s.S[K_old:].any()
    else:
        assert not s.S[K_old:].any()
    assert np.array_equal(s.ids, np.concatenate([np.arange(11, 11 + K_old), 10 + K_old + np.arange(1, K_new + 1)]))
    assert s.tags.shape == (K_old + K_new,) and s.tags.dtype == np.uint16 and s.P["k_ids"] == 10 + K_old + K_new
    # every session was opened with the factors, the filter of the scaled values, on the low-resolution grid; the observer got Yds, the images are resized back
    assert len(eng.opened) == len(video.owned) == len(opened)
    psf = seed_psf(c["gSig"] / ssub, float(gz), True)
    for (pid, fs, ft, psf_got, grid, Ts), idx in zip(eng.opened, video.order):
        pp = [int(x) for x in video.patch_pos[idx]]
        nr, nc = pp[1] - pp[0] + 1, pp[3] - pp[2] + 1
        assert (fs, ft, grid, Ts) == (ssub, tsub, (-(-nr // ssub), -(-nc // ssub)), T // tsub) and np.array_equal(psf_got, psf)
        data = opened[idx]
        assert "Yres" not in data and data["Yds"].shape == (Ts, grid[0] * grid[1])
        low = np.asarray(data["Cn"], dtype=np.float64).reshape(grid, order="F")
        want = dso.imresize(low, (nr, nc)) if ssub != 1 else low
        assert np.abs(Cn[pp[0] - 1:pp[1], pp[2] - 1:pp[3]] - want).max() <= 1e-12
    assert all("peel" not in q for q in eng.p.values())
    with pytest.raises(NotImplementedError):
        s.initComponents_residual_parallel(save_avi=True)


@pytest.mark.parametrize("name", ["B", "D"])
def test_seeds_land_on_the_low_resolution_cell(name):
    """the forced-seed run: FOV pixels -> the cell ((r - r0) // ssub, (c - c0) // ssub) of the patch that holds them; the oracle's forced run is retraced"""
    c = dc.CASES[name]
    ora = dc.oracle(name, True)
    seeds = [tuple(int(x) for x in r) for r in dc.oracle(name)["center"]]
    eng, video, s, A0 = _host_run(name)
    tried = {}
    s._init_observer = lambda idx, kind, data: tried.setdefault(idx, []).append((data["r"], data["c"])) if kind == "extract" else None
    center, _, _ = s.initComponents_residual_parallel(K=c.get("Kmax"), min_corr=c["min_corr"], min_pnr=c["min_pnr"], seeds=seeds)
    assert np.array_equal(center, ora["center"])
    for idx in video.order:
        pp = [int(x) for x in video.patch_pos[idx]]
        mine = [((r - pp[0]) // c["ssub"], (q - pp[2]) // c["ssub"]) for (r, q) in seeds if pp[0] <= r <= pp[1] and pp[2] <= q <= pp[3]]
        assert tried.get(idx, []) == mine, (idx, tried.get(idx), mine)
    assert sum(len(v) for v in tried.values()) == len(seeds)


# ---- 4. refusals -----------------------------------------------------------------------------------------------------------------------------------------------------
def test_refusals():
    from cnmf_e_amd.sources2d import Options
    c = dc.CASES["A"]
    eng, video, s, _ = _host_run("A")
    type(eng).supports_init_residual_ds = False
    try:
        with pytest.raises(NotImplementedError, match="supports_init_residual_ds"):
            s.initComponents_residual_parallel()
    finally:
        type(eng).supports_init_residual_ds = True
    s.options = dc.options("A", **{})
    s.options.tsub = 3                                                     # swapped in after construction
    with pytest.raises(NotImplementedError, match="constructed with ssub = 2, tsub = 2"):
        s.initComponents_residual_parallel()
    eng, video, s, _ = _host_run("A", options=Options(ring_radius=c["r"], gSig=c["gSig"], gSiz=c["gSiz"], maxIter=3, bd=dc.BD, tsub=7))
    with pytest.raises(ValueError, match=r"floor\(402 / 7\) = 57"):
        s.initComponents_residual_parallel()


def test_no_fitted_background_is_refused_with_factors_only():
    """before the first update_background_parallel W is the ring's indicator: the down-sampled second pass refuses, the full-resolution one runs as it did"""
    from cnmf_e_amd.sources2d import Options, PatchedVideo, Sources2D
    c = dc.CASES["A"]
    f, Y, A0, C0 = dc.inputs("A")
    for opt, refused in ((dict(ssub=c["ssub"], tsub=c["tsub"]), True), ({}, False)):
        eng = _double()
        eng.gSig, eng.gSiz = c["gSig"], c["gSiz"]
        video = PatchedVideo(c["dims"][0], c["dims"][1], c["T"], dc.pdims(c), c["r"], eng)
        video.upload_from_full(Y)
        s = Sources2D(video, Options(ring_radius=c["r"], gSig=c["gSig"], gSiz=c["gSiz"], bd=dc.BD, **opt), A0, C0, f.sn)
        if refused:
            with pytest.raises(NotImplementedError, match="before the first update_background_parallel"):
                s.initComponents_residual_parallel(K=1)
            assert not eng.opened and all("peel" not in q for q in eng.p.values())
            s.update_background_parallel()
        s.initComponents_residual_parallel(K=1)
        assert all("peel" not in q for q in eng.p.values())
    assert not eng.opened
