"""The host mirror of background_model = 'svd' (cnmf_e_amd.sources2d) on a NumPy engine (tests/svd_fake_engine.py): the constructor, the three update methods against
the oracle loop (tests/svd_bg_oracle.SvdOracleLoop), the skip rule, reconstruct_background and every refusal."""
import warnings

import numpy as np
import pytest
import scipy.sparse as sp

import svd_bg_cases as sc
import svd_bg_oracle as so
from fake_engine import FakeEngine
from svd_fake_engine import SvdFakeEngine

from cnmf_e_amd.sources2d import Options, PatchedVideo, Sources2D


def _make(case, eng=None, **opt):
    eng = eng or SvdFakeEngine()
    v = PatchedVideo(case["d1"], case["d2"], case["T"], case["patch"], case["halo"], eng)
    v.upload_from_full(case["Y"])
    o = Options(ring_radius=case["halo"], background_model=opt.pop("background_model", "svd"), nb=case["nb"], **opt)
    return Sources2D(v, o, case["A"], case["C"], np.ones(case["d1"] * case["d2"], np.float32)), v, eng


def _oracle(case, **kw):
    Y = case["Y"].T.astype(np.float64).reshape(case["d1"], case["d2"], case["T"], order="F")
    return so.SvdOracleLoop(Y, case["d1"], case["d2"], case["T"], case["patch"], case["halo"], case["A"], case["C"], nb=case["nb"], **kw)


def rel(a, b):
    a = np.asarray(a, dtype=np.float64); b = np.asarray(b, dtype=np.float64)
    return float(np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-30))


@pytest.mark.parametrize("model", ["svd", "SVD", "Svd"])
def test_constructor_accepts_svd_without_any_ring_call(model):
    case = sc.make_case("quad", 2)
    s, v, eng = _make(case, background_model=model)
    assert s.bg_model == "svd"
    assert not any(c[0] == "ring_init" for c in eng.calls)
    for idx in v.order:                                                     # zero at first: b d x nb, f nb x T, b0 d
        n = v.patch_pix[idx].size
        assert s.get_b(idx).shape == (n, 2) and s.get_f(idx).shape == (2, case["T"]) and s.get_b0(idx).shape == (n,)
        assert not s.get_b(idx).any() and not s.get_f(idx).any() and not s.get_b0(idx).any()


def test_constructor_refusals():
    case = sc.make_case("small", 1)
    with pytest.raises(ValueError):
        _make(case, background_model="nmf")
    with pytest.raises(ValueError):
        _make(case, background_model="rings")
    with pytest.raises(NotImplementedError, match="svd"):
        _make(case, eng=FakeEngine())                                       # an engine that does not declare supports_bg_svd
    v = PatchedVideo(case["d1"], case["d2"], case["T"], case["patch"], case["halo"], SvdFakeEngine())
    v.upload_from_full(case["Y"])
    with pytest.raises(NotImplementedError, match="dist_group"):
        Sources2D(v, Options(ring_radius=case["halo"], background_model="svd"), case["A"], case["C"], np.ones(120, np.float32), dist_group=object())

    class Laned(SvdFakeEngine):
        def get_option(self, name, default):
            return 2 if name == "lanes" else default
    with pytest.raises(NotImplementedError, match="lanes"):
        _make(case, eng=Laned())
    bad = dict(case); bad["nb"] = 9
    with pytest.raises(ValueError, match="nb"):
        _make(bad)
    # ring mode is what it was: the ring is initialised, the svd accessors are not its
    s, v, eng = _make(case, background_model="ring")
    assert s.bg_model == "ring" and any(c[0] == "ring_init" for c in eng.calls)
    with pytest.raises(NotImplementedError):
        s.get_b(v.order[0])


@pytest.mark.parametrize("alg", ["hals", "nnls"])
def test_two_iterations_equal_the_oracle_loop(alg):
    """2 x 2 patches, background -> spatial -> temporal twice.  The double computes in float64 what the oracle computes; the host keeps A and C in fp32 between the
    calls (as with the real engine), so the agreement is that of fp32 storage, 6e-8 per value, not of the arithmetic."""
    case = sc.make_case("quad", 2)
    s, v, eng = _make(case, spatial_algorithm=alg, maxIter=3)
    o = _oracle(case, spatial_algorithm=alg, maxIter=3)
    for it in range(2):
        s.update_background_parallel(); o.update_background_parallel()
        for idx in v.order:
            assert rel(s.get_b(idx) @ s.get_f(idx) + s.get_b0(idx)[:, None], o.b[idx] @ o.f[idx] + o.b0[idx][:, None]) <= 1e-6, (it, idx)
        assert s.A_prev is s.A and s.C_prev is s.C                         # update_background_parallel.m:316-317
        s.update_spatial_parallel(); o.update_spatial_parallel()
        Ag, Ar = s.A.toarray(), o.A.toarray()
        assert ((Ag != 0) != (Ar != 0)).sum() == 0, it
        assert rel(Ag, Ar) <= 1e-5, (it, rel(Ag, Ar))
        s.update_temporal_parallel(); o.update_temporal_parallel()
        assert rel(s.C, o.C) <= 1e-5 and rel(s.C_raw, o.C_raw) <= 1e-5, (it, rel(s.C, o.C))
    assert rel(s.reconstruct_background(), o.reconstruct_background()) <= 1e-6
    part = s.reconstruct_background(frame_range=(10, 20))
    assert part.shape == (48, 48, 11) and rel(part, o.reconstruct_background()[:, :, 9:20]) <= 1e-6
    # neurons are selected by the PATCH rectangle: the neuron that straddles the border of patches (0, 0) and (1, 0) belongs to both, none to the right-hand patches
    straddler = 1
    rows = lambda idx: s.A.tocsr()[v.patch_pix[idx]]
    assert rows((0, 0))[:, straddler].nnz > 0 and rows((1, 0))[:, straddler].nnz > 0
    assert rows((0, 1)).nnz == 0 and rows((1, 1)).nnz == 0
    assert [k for k in s._slice(s.A, (0, 0), "patch")[0]] == [0, 1, 3] and [k for k in s._slice(s.A, (1, 0), "patch")[0]] == [1, 2]
    # ... so the updates ask for the residual of the two left-hand patches only, once per patch and update
    asked = [c[1] for c in eng.calls if c[0] == "residual_lowrank"]
    assert sorted(set(asked)) == [v.pid[(0, 0)], v.pid[(1, 0)]] and len(asked) == 2 * 2 * 2


def test_skip_rule_reads_patch_one_only():
    """update_background_parallel.m:145,188-199: after the first run a patch without a neuron in its block keeps b, f, b0; the first run fits every patch"""
    case = sc.make_case("quad", 1)
    s, v, eng = _make(case)
    s.update_background_parallel()
    assert sorted(c[1] for c in eng.calls if c[0] == "bg_svd_fit") == [0, 1, 2, 3]                  # flag_first: b{1} is all zero
    empty = [idx for idx in v.order if s._slice(s.A, idx, "block")[0].size == 0]
    assert empty == [(0, 1), (1, 1)]
    marked = {idx: (np.full_like(s.get_b(idx), 7.0), np.full_like(s.get_f(idx), 3.0), np.full_like(s.get_b0(idx), 5.0)) for idx in empty}
    for idx, (b, f, b0) in marked.items():
        s.set_bg_svd(idx, b, f, b0)
    eng.calls.clear()
    s.update_background_parallel()
    assert sorted(c[1] for c in eng.calls if c[0] == "bg_svd_fit") == [v.pid[(0, 0)], v.pid[(1, 0)]]
    for idx, (b, f, b0) in marked.items():
        assert np.array_equal(s.get_b(idx), b) and np.array_equal(s.get_f(idx), f) and np.array_equal(s.get_b0(idx), b0)
    # b{1} back to zero: a first run again, for EVERY patch -- the rule reads patch 1 only
    first = v.order[0]
    s.set_bg_svd(first, np.zeros_like(s.get_b(first)), s.get_f(first), s.get_b0(first))
    eng.calls.clear()
    s.update_background_parallel()
    assert sorted(c[1] for c in eng.calls if c[0] == "bg_svd_fit") == [0, 1, 2, 3]


def test_nb_zero_and_cap_warning():
    case = sc.make_case("small", 0)
    s, v, eng = _make(case)
    s.update_background_parallel()
    idx = v.order[0]
    assert s.get_b(idx).shape == (120, 0) and s.get_f(idx).shape == (0, case["T"])
    Yb = case["Y"].T.astype(np.float64)
    ref = Yb.mean(axis=1) - case["A"].astype(np.float64) @ case["C"].astype(np.float64).mean(axis=1)
    assert np.allclose(s.get_b0(idx), ref)
    assert np.allclose(s.reconstruct_background()[:, :, 0].reshape(-1, order="F"), ref, rtol=1e-6)
    eng.max_iter_hit = True                                                 # a fit that hits the iteration cap is a warning, not an error
    with pytest.warns(RuntimeWarning):
        s.update_background_parallel()


def test_everything_that_reads_the_ring_background_is_refused():
    case = sc.make_case("small", 1)
    s, v, eng = _make(case)
    s.update_background_parallel()
    idx = v.order[0]
    for call in (s.compute_RSS, s.initComponents_residual_parallel, s.initTemporal, s.extract_DF_F_endoscope, lambda: next(s.demixed_frames()), s.show_demixed_video,      # (demixed_frames is a generator: it speaks at the first chunk)
                 lambda: s.update_spatial_parallel(update_sn=True), lambda: s.get_W(idx), lambda: s.init_residual(idx), lambda: s.set_b0(idx, np.zeros(120)),
                 lambda: s.set_W(idx, np.zeros(3))):
        with pytest.raises(NotImplementedError, match="svd"):
            call()
    from cnmf_e_amd.batch import Sources2DBatch
    with pytest.raises(NotImplementedError, match="svd"):
        Sources2DBatch([s], s.options)


def test_what_does_not_read_the_background_still_works():
    case = sc.make_case("one", 1)
    s, v, eng = _make(case)
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        s.update_background_parallel()
        s.update_spatial_parallel()
        s.update_temporal_parallel()
    K = s.A.shape[1]
    assert s.A.shape[1] == K and s.C.shape == (K, case["T"])
    s.delete([0])                                                          # (orderROIs, merges and tags need the real engine: tests/test_gpu_svd_bg.py)
    assert s.A.shape[1] == K - 1 and s.C.shape[0] == K - 1
    assert sp.issparse(s.A)
