"""background_model = 'svd' on the device against the float64 oracle (tests/svd_bg_oracle.py) on the cases of tests/svd_bg_cases.py:

    one    40 x 36, T = 203, one patch     d_b = 1440 > T, T mod 4 = 3, d_b no multiple of 256, rows no multiple of 16
    small  12 x 10, T = 301                d_b = 120 < T
    quad   48 x 48, T = 256, 2 x 2 patches with a halo: ind_patch is a strict interior of the block, a neuron straddles a patch border, two blocks hold no neuron

Bounds.  The fit's error against the oracle is MEASURED (printed by every test; DESIGN.md section 8 records it) and the bounds below are at most 10x the largest value
observed on MI355X, the rule of that section.  The residual kernel's bound is one fp32 rounding of the exact value.  The updates use the tolerances of
tests/test_gpu_parity.py, the end-to-end run those of tests/test_gpu_zconfigs.py for the same quantities."""
import warnings

import numpy as np
import pytest
import scipy.sparse as sp

import cnmfe_oracle as orc
import svd_bg_cases as sc
import svd_bg_oracle as so
from parity_util import rel

pytestmark = pytest.mark.gpu

# Observed on MI355X, maxima over every case, patch and nb of this file: rel(b f) 3.4e-9, the singular values 4.9e-10, |b0 - b0_ref| / max|Ymean|
# 1.4e-16, |f f' - I| 1.6e-15; reconstruct_background (fp32 output, dominated by b0) 2.5e-8.  The bounds are 10x those.
BOUND_BF = 3e-8
BOUND_S = 4.9e-9
BOUND_B0 = 1.4e-15
BOUND_BG_F32 = 2.4e-7
BOUND_ORTH = 1.6e-14


@pytest.fixture(scope="module")
def eng():
    from cnmf_e_amd.engine import Engine
    e = Engine(0)
    yield e
    e.close()


def _video(eng, case):
    from cnmf_e_amd.sources2d import PatchedVideo
    v = PatchedVideo(case["d1"], case["d2"], case["T"], case["patch"], case["halo"], eng)
    v.upload_from_full(case["Y"])
    return v


def _fit_inputs(case, v, idx):
    Yb, ind, A_b, C_b = sc.block_inputs(case, v.block_pix[idx])
    ip = np.zeros(v.block_pix[idx].size, dtype=bool); ip[v.ind_patch[idx]] = True
    return Yb, ind, (A_b if ind.size else None), (np.ascontiguousarray(C_b) if ind.size else None), ip


@pytest.mark.parametrize("name,neurons", sc.CASES)
@pytest.mark.parametrize("nb", [0, 1, 2, 3])
def test_fit_against_oracle(eng, observed, name, neurons, nb):
    case = sc.make_case(name, nb, neurons)
    v = _video(eng, case)
    obs = observed.setdefault("svd_bg_fit", {})
    for idx in v.order:
        pid = v.pid[idx]
        Yb, ind, A_b, C_b, ip = _fit_inputs(case, v, idx)
        eng.bind_traces(None)
        with warnings.catch_warnings():
            warnings.simplefilter("error")                                   # a fit that hits the cap would warn
            st = eng.bg_svd_fit(pid, nb, A_b, C_b)
        b, f, b0 = eng.bg_svd_get(pid)
        br, fr, b0r = so.fit_svd_model(Yb, nb, A_b, C_b, ind_patch=ip)
        assert b.shape == br.shape and f.shape == fr.shape and b0.shape == b0r.shape
        e_b0 = float(np.abs(b0 - b0r).max() / np.abs(Yb.mean(axis=1)).max())
        key = "%s_%d_nb%d_%d%d" % (name, neurons, nb, idx[0], idx[1])
        assert st["converged"] and st["nb"] == nb
        if nb:
            e_bf = rel(b @ f, br @ fr)                                      # the product: b and f singly are defined up to a sign
            e_or = float(np.abs(f @ f.T - np.eye(nb)).max())
            print("svd fit %s: rel(b f) %.2e  b0 %.2e  |f f' - I| %.2e  iterations %d passes %d residual %s s %s"
                  % (key, e_bf, e_b0, e_or, st["iterations"], st["passes"], np.array2string(st["residual"], precision=1), np.array2string(st["s"], precision=4)))
            obs[key] = dict(bf=e_bf, b0=e_b0, orth=e_or, iterations=st["iterations"], residual=float(st["residual"].max()))
            assert e_bf <= BOUND_BF and e_or <= BOUND_ORTH, (key, e_bf, e_or)
            assert np.all(np.diff(st["s"]) <= 0) and np.all(st["s"] > 0)
            e_s = rel(st["s"], so.singular_values(Yb, A_b, C_b)[:nb])
            print("svd fit %s: rel(s) %.2e" % (key, e_s))
            assert e_s <= BOUND_S, (key, e_s)
            # sign: the entry of largest magnitude of every u_i is positive -- on a one-patch case the patch rows are the block rows
            if ip.all():
                assert all(b[np.argmax(np.abs(b[:, i])), i] > 0 for i in range(nb))
        else:
            print("svd fit %s: b0 %.2e" % (key, e_b0))
            obs[key] = dict(b0=e_b0)
            assert st["passes"] == 0
        assert e_b0 <= BOUND_B0, (key, e_b0)
        # two runs give equal bits; a bound C and the same C uploaded give equal bits
        eng.bg_svd_fit(pid, nb, A_b, C_b)
        again = eng.bg_svd_get(pid)
        assert all(np.array_equal(x, y) for x, y in zip((b, f, b0), again))
        if C_b is not None:
            eng.bind_traces(C_b)
            eng.bg_svd_fit(pid, nb, A_b, C_b)                               # (the bound matrix by identity: (NULL, CNMFE_BOUND))
            bound = eng.bg_svd_get(pid)
            assert all(np.array_equal(x, y) for x, y in zip((b, f, b0), bound))
            # ... and rows of a larger bound matrix, in another order there: (rows, CNMFE_BOUND_ROWS), the form Sources2D passes for a patch's neurons
            from cnmf_e_amd.engine import BoundRows
            perm = np.arange(C_b.shape[0])[::-1]
            big = np.ascontiguousarray(np.vstack([np.full((1, case["T"]), 7.0, np.float32), C_b[perm], np.full((2, case["T"]), -3.0, np.float32)]))
            rows = 1 + np.argsort(perm)                                     # big[rows] == C_b
            assert np.array_equal(big[rows], C_b)
            eng.bind_traces(big)
            eng.bg_svd_fit(pid, nb, A_b, BoundRows(big, rows))
            by_rows = eng.bg_svd_get(pid)
            eng.bind_traces(None)
            assert all(np.array_equal(x, y) for x, y in zip((b, f, b0), by_rows))


@pytest.mark.parametrize("name", list(sc.SHAPES))
@pytest.mark.parametrize("nb", [0, 3])
def test_residual_kernel_after_set(eng, name, nb):
    """k_lowrank_resid alone: a transplanted b, f, b0, the exported Ysig against float64.  Exact value: Yc + (ymean_f - b0) - b f with Yc = fl32(Y - ymean_f), the video as
    the engine holds it; the result is that value rounded ONCE to fp32: |error| <= 2^-24 |exact| <= 2^-23 (|Yc| + |Ymean - b0| + |b f|) with room for the fp64 sums."""
    case = sc.make_case(name, 1)
    v = _video(eng, case)
    rng = np.random.default_rng(7)
    for idx in v.order:
        pid = v.pid[idx]
        d = v.patch_pix[idx].size
        b = rng.normal(0.0, 20.0, (d, nb)); f = rng.normal(0.0, 1.0, (nb, case["T"])); b0 = case["Y"][:, v.patch_pix[idx]].mean(axis=0, dtype=np.float64) + rng.normal(0.0, 3.0, d)
        eng.bg_svd_set(pid, b, f, b0)
        got = eng.residual_lowrank(pid, want=True).T.astype(np.float64)                              # d x T
        back = eng.bg_svd_get(pid)
        assert np.array_equal(back[0], b) and np.array_equal(back[1], f) and np.array_equal(back[2], b0)
        ymf = eng.ymean(pid)[v.ind_patch[idx]].astype(np.float32)
        Yc = (case["Y"][:, v.patch_pix[idx]] - ymf[None, :]).T.astype(np.float64)                   # fp32 subtraction, as k_center4
        dl = ymf.astype(np.float64) - b0
        exact = Yc + dl[:, None] - b @ f
        bound = 2.0 ** -23 * (np.abs(Yc) + np.abs(dl)[:, None] + np.abs(b @ f))
        err = np.abs(got - exact)
        worst = float((err / np.maximum(bound, 1e-300)).max())
        print("lowrank_resid %s nb %d patch %s: max error / bound %.3f" % (name, nb, idx, worst))
        assert np.all(err <= bound), (name, idx, worst)
        assert np.all(err[:, -3:] <= bound[:, -3:]) and np.all(err[-1] <= bound[-1])                  # the T mod 4 tail frames, the last pixel


def _updates_setup(eng, name, nb=2):
    case = sc.make_case(name, nb)
    v = _video(eng, case)
    out = []
    for idx in v.order:
        pid = v.pid[idx]
        Yb, ind, A_b, C_b, ip = _fit_inputs(case, v, idx)
        b, f, b0 = so.fit_svd_model(Yb, nb, A_b, C_b, ind_patch=ip)
        eng.bg_svd_set(pid, b, f, b0)
        ysig = Yb[ip] - (b @ f + b0[:, None])                               # the oracle's Ysig
        out.append((idx, pid, ysig))
    return case, v, out


@pytest.mark.parametrize("alg", ["hals", "hals_thresh", "nnls"])
@pytest.mark.parametrize("name", ["one", "quad"])
def test_update_spatial_under_svd(eng, name, alg):
    from cnmf_e_amd.sources2d import determine_search_location
    case, v, patches = _updates_setup(eng, name)
    IND = determine_search_location(case["A"], case["d1"], case["d2"])
    rng = np.random.default_rng(3)
    C0 = np.maximum(case["C"] + rng.normal(0.0, 0.3, case["C"].shape), 0).astype(np.float32)
    done = 0
    for idx, pid, ysig in patches:
        pp = v.patch_pix[idx]
        INDp = IND.tocsr()[pp]
        ind = np.nonzero(np.asarray(INDp.sum(axis=0)).ravel() > 0)[0]
        if ind.size == 0:
            continue
        INDp = INDp[:, ind].tocsc(); A_p = case["A"].tocsr()[pp][:, ind].tocsc().astype(np.float32); C_p = C0[ind]
        sn = np.full(pp.size, sc.NOISE, dtype=np.float32)
        eng.residual_lowrank(pid)
        got = eng.update_spatial(pid, alg, A_p, C_p, INDp, sn, 20 if alg == "nnls" else 3).toarray()
        if alg == "hals":
            ref = orc.HALS_spatial(ysig, A_p, C_p, INDp, 3)
        elif alg == "hals_thresh":
            ref = orc.HALS_spatial_thresh(ysig, A_p, C_p, INDp, 3, sn)
        else:
            ref = orc.nnls_spatial(ysig, A_p, C_p, INDp, 20)
        mism = (got != 0) != (ref != 0)
        e = rel(got[~mism], ref[~mism])
        print("spatial %s %s %s: mismatches %d rel %.2e" % (name, alg, idx, mism.sum(), e))
        assert mism.sum() == 0, mism.sum()
        assert e <= 3e-6, e                                                 # tests/test_gpu_parity.py::test_update_spatial_parity
        done += 1
    assert done >= (1 if name == "one" else 2)


@pytest.mark.parametrize("name", ["one", "quad"])
def test_hals_temporal_under_svd(eng, name):
    case, v, patches = _updates_setup(eng, name)
    rng = np.random.default_rng(4)
    C0 = np.maximum(case["C"] + rng.normal(0.0, 0.3, case["C"].shape), 0).astype(np.float32)
    for idx, pid, ysig in patches:
        pp = v.patch_pix[idx]
        A_p = case["A"].tocsr()[pp].tocsc().astype(np.float32)
        ind = np.nonzero(np.asarray(A_p.sum(axis=0)).ravel() > 0)[0]
        if ind.size == 0:
            continue                                                        # (update_temporal_parallel.m:123: the caller's skip)
        A_p = A_p[:, ind]
        eng.residual_lowrank(pid)
        Cg, Crawg, aa = eng.hals_temporal(pid, A_p, C0[ind], 5)
        Cr, Crawr, _ = orc.HALS_temporal(ysig, A_p.astype(np.float64), C0[ind], 5, None)
        print("temporal %s %s: rel C %.2e C_raw %.2e" % (name, idx, rel(Cg, Cr), rel(Crawg, Crawr)))
        assert rel(Cg, Cr) <= 2e-6 and rel(Crawg, Crawr) <= 2e-6             # tests/test_gpu_parity.py::test_hals_temporal_parity
        Crg, aag = eng.fast_temporal(pid, A_p)
        aar, Crr = orc.fast_temporal(ysig, A_p.astype(np.float64))
        assert rel(Crg, Crr) <= 2e-6 and np.allclose(aag, aar, rtol=1e-5)


def test_hals_temporal_deconv_under_svd(eng):
    import oasis_oracle as oo
    case, v, patches = _updates_setup(eng, "small")
    (idx, pid, ysig), = patches
    A_p = case["A"].tocsc().astype(np.float32)
    eng.residual_lowrank(pid)
    Cg, Crawg, Sg, sng, parsg, aa = eng.hals_temporal_deconv(pid, A_p, case["C"], 2, None)
    Cr, Crawr, Sr, snr, parsr = oo.HALS_temporal_deconv(ysig, A_p.astype(np.float64), case["C"], 2)
    print("temporal deconv: sn %.2e pars %.2e C %s" % (np.abs(sng / snr - 1).max(), np.abs(parsg - np.array(parsr, dtype=np.float64)).max(),
                                                       [rel(Cg[k], Cr[k]) for k in range(Cg.shape[0])]))
    assert np.allclose(sng, snr, rtol=5e-6)                                  # tests/test_gpu_parity.py::test_hals_temporal_deconv_parity
    assert np.allclose(parsg, np.array(parsr, dtype=np.float64), atol=2e-6), (parsg, parsr)
    for k in range(Cg.shape[0]):
        assert rel(Cg[k], Cr[k]) <= 5e-6 and rel(Crawg[k], Crawr[k]) <= 5e-6, (k, rel(Cg[k], Cr[k]), rel(Crawg[k], Crawr[k]))


def test_sources2d_two_iterations_against_oracle_loop(eng, observed):
    from cnmf_e_amd.sources2d import Options, Sources2D
    case = sc.make_case("quad", 2)
    v = _video(eng, case)
    s = Sources2D(v, Options(ring_radius=case["halo"], background_model="svd", nb=2, maxIter=5), case["A"], case["C"], np.ones(48 * 48, np.float32))
    Y = case["Y"].T.astype(np.float64).reshape(48, 48, case["T"], order="F")
    o = so.SvdOracleLoop(Y, 48, 48, case["T"], case["patch"], case["halo"], case["A"], case["C"], nb=2, maxIter=5)
    obs = observed.setdefault("svd_bg_loop", {})
    for it in range(2):
        with warnings.catch_warnings():
            warnings.simplefilter("error")
            stats = s.update_background_parallel()
        o.update_background_parallel()
        assert sorted(stats) == (sorted(v.order) if it == 0 else [(0, 0), (1, 0)])                    # the skip rule: the right-hand blocks hold no neuron
        e_bg = rel(s.reconstruct_background(), o.reconstruct_background())
        s.update_spatial_parallel(); o.update_spatial_parallel()
        Ag, Ar = s.A.toarray(), o.A.toarray()
        mism = (Ag != 0) != (Ar != 0)
        e_a = rel(Ag[~mism], Ar[~mism])
        s.update_temporal_parallel(); o.update_temporal_parallel()
        e_c, e_cr = rel(s.C, o.C), rel(s.C_raw, o.C_raw)
        print("svd loop %d: background %.2e  A mismatches %d rel %.2e  C %.2e C_raw %.2e" % (it, e_bg, mism.sum(), e_a, e_c, e_cr))
        obs["it%d" % it] = dict(background=e_bg, A=e_a, mism=int(mism.sum()), C=e_c, C_raw=e_cr)
        assert e_bg <= BOUND_BG_F32, (it, e_bg)
        assert mism.sum() == 0 and e_a <= 1e-6, (it, mism.sum(), e_a)        # tests/test_gpu_zconfigs.py: A
        assert e_c <= 5e-6 and e_cr <= 5e-6, (it, e_c, e_cr)                # ... C, C_raw
    # what does not read the background keeps working on the real engine
    K = s.A.shape[1]
    s.orderROIs("snr")
    assert s.A.shape[1] == K
    for call in (s.compute_RSS, s.extract_DF_F_endoscope, s.initTemporal):
        with pytest.raises(NotImplementedError, match="svd"):
            call()


def test_state_rules(eng):
    from cnmf_e_amd._lib import CnmfeError
    case = sc.make_case("small", 2)
    v = _video(eng, case)
    idx = v.order[0]; pid = v.pid[idx]
    Yb, ind, A_b, C_b, ip = _fit_inputs(case, v, idx)
    A_p = case["A"].tocsc().astype(np.float32)
    with pytest.raises(CnmfeError, match="error -4"):                       # no background yet
        eng.residual_lowrank(pid)
    eng.bg_svd_fit(pid, 2, A_b, C_b)
    with pytest.raises(CnmfeError, match="error -4"):                       # an update before any cnmfe_residual_lowrank
        eng.hals_temporal(pid, A_p, case["C"], 2)
    eng.residual_lowrank(pid)
    first = eng.hals_temporal(pid, A_p, case["C"], 2)[1]
    with pytest.raises(CnmfeError, match="error -5"):                       # compute_RSS / reconstruct_background serve the ring's residual only
        eng.compute_rss(pid, A_p, case["C"], np.zeros(120, np.float32), np.zeros(120, np.float32))
    eng.residual_lowrank(pid)                                               # still valid: nothing to do, same values
    assert np.array_equal(first, eng.hals_temporal(pid, A_p, case["C"], 2)[1])
    eng.bg_svd_fit(pid, 2, A_b, C_b)                                        # a fit invalidates the residual
    with pytest.raises(CnmfeError, match="error -4"):
        eng.hals_temporal(pid, A_p, case["C"], 2)
    eng.residual_lowrank(pid)
    eng.bg_svd_set(pid, *eng.bg_svd_get(pid))                               # ... and so does a set
    with pytest.raises(CnmfeError, match="error -4"):
        eng.fast_temporal(pid, A_p)
    with pytest.raises(CnmfeError, match="error -5"):
        eng.bg_svd_fit(pid, 9, A_b, C_b)
    # an upload of the video invalidates the residual; b, f, b0 stay, and the same video gives the same residual again
    eng.residual_lowrank(pid)
    before = eng.residual_lowrank(pid, want=True)
    eng.upload_block(pid, case["Y"][:, v.block_pix[idx]])
    with pytest.raises(CnmfeError, match="error -4"):
        eng.hals_temporal(pid, A_p, case["C"], 2)
    assert np.array_equal(before, eng.residual_lowrank(pid, want=True))
    eng.hals_temporal(pid, A_p, case["C"], 2)
    # nb above min(d_b, T): a 2 x 2 block has rank 4 at most
    eng.create_patch(900, [1, 2, 1, 2], [1, 2, 1, 2], 2, 2, 16)
    with pytest.raises(CnmfeError, match="error -5"):
        eng.bg_svd_fit(900, 5)
    # the iteration cap set to 1: a clean not-converged report, no fault, no NaN
    eng.set_option("bg_svd_max_iter", 1)
    try:
        with pytest.warns(RuntimeWarning):
            st = eng.bg_svd_fit(pid, 2, A_b, C_b)
        assert not st["converged"] and st["iterations"] == 1 and st["passes"] == 3
        assert all(np.isfinite(x).all() for x in eng.bg_svd_get(pid)) and np.isfinite(st["residual"]).all()
    finally:
        eng.set_option("bg_svd_max_iter", 40)
    st = eng.bg_svd_fit(pid, 2, A_b, C_b)
    assert st["converged"]
