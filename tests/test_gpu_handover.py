"""The hand-over from the spatial to the temporal update (engine option temporal_early).

With the option on, the temporal projection U = B' Yc is queued behind the spatial update's connectivity kernel, from the post-processed result where it lies on
the device and block lists built from the MASK's pattern (a superset of A's: stored zeros, all-zero panel columns), and the Gauss-Seidel levels are queued without
the host wait for A'A (aa and its check taken on the device).  Neither may change a value: every comparison here is np.array_equal between temporal_early = 1
(or 2 / 3: one half alone) and temporal_early = 0 on the same seeded input, after two full iterations.  A positive case also asserts, through the library's
counters, that the early path served the update -- a silent fallback cannot pass -- and a fallback case that it did not.

The wait in front of the levels is kept when a footprint term over more than 512 traces was applied (its list kernel may overflow); no case here has that many
neurons, so the kept wait is exercised through temporal_early = 2, which keeps it always."""
import numpy as np
import pytest
import scipy.sparse as sp

pytestmark = pytest.mark.gpu

TINY = dict(dims=(96, 96), pdims=None, T=600, K=18, r=15, seed=5)          # bench.py's `tiny`
COUNTERS = ("temporal_early_hits", "temporal_early_drops", "temporal_early_declined", "temporal_nowait")


def _factors(dims, T, K, seed, fkw):
    from cnmf_e_amd import synth
    f = synth.make_factors(dims[0], dims[1], T, K, seed, **(fkw or {}))
    return f, synth.make_video(f, np.float32), f.A_init, f.C_init


def _spurious(dims, T, K, seed, fkw):
    """the factors plus ONE spurious neuron: a 3 x 3 footprint on the background pixel farthest from every real footprint, with a trace of rectified white noise.
    HALS_spatial_thresh's 3-sigma test leaves none of its pixels (found with oracle/cnmfe_oracle.py: seeds 5, 6, 7 and 10 of this size give an all-zero column)"""
    from scipy.ndimage import distance_transform_edt
    f, Y, A0, C0 = _factors(dims, T, K, seed, fkw)
    d1, d2 = dims
    occ = np.asarray(A0.sum(axis=1)).ravel().reshape(d1, d2, order="F") > 0
    dist = distance_transform_edt(~occ); dist[:6] = 0; dist[-6:] = 0; dist[:, :6] = 0; dist[:, -6:] = 0
    rr, cc = np.unravel_index(np.argmax(dist), dist.shape)
    col = np.zeros(d1 * d2, np.float32)
    for dr in (-1, 0, 1):
        for dc in (-1, 0, 1):
            col[(cc + dc) * d1 + rr + dr] = 0.3
    A = sp.hstack([sp.csc_matrix(A0), sp.csc_matrix(col[:, None])]).tocsc().astype(np.float32)
    ck = np.maximum(np.random.default_rng(1000 + seed).normal(0.0, 1.0, T), 0.0).astype(np.float32)
    return f, Y, A, np.vstack([C0, ck[None]]).astype(np.float32)


def _run(te, dims, pdims, T, K, r, seed, opt_kw=None, opts=None, lanes=1, fkw=None, make=_factors, iters=2, between=None):
    """`iters` full iterations under temporal_early = te on a fresh engine -> (outputs, counters).  between(s, eng, it): called between the spatial and the temporal
    update of iteration `it`"""
    from cnmf_e_amd.engine import Engine
    from cnmf_e_amd.sources2d import PatchedVideo, Sources2D, Options
    f, Y, A0, C0 = make(dims, T, K, seed, fkw)
    eng = Engine(0)
    try:
        if lanes > 1:
            eng.set_option("lanes", lanes)
        eng.set_option("temporal_early", te)
        for k, v in (opts or {}).items():
            eng.set_option(k, v)
        video = PatchedVideo(dims[0], dims[1], T, pdims or list(dims), r, eng)
        video.upload_from_full(Y)
        kw = dict(spatial_algorithm="hals", maxIter=5); kw.update(opt_kw or {})
        s = Sources2D(video, Options(ring_radius=r, **kw), A0, C0, f.sn)
        for it in range(iters):
            s.update_background_parallel()
            s.update_spatial_parallel()
            if between:
                between(s, eng, it)
            s.update_temporal_parallel()
        out = dict(A=s.A.toarray(), C=np.asarray(s.C, dtype=np.float32).copy(), C_raw=np.asarray(s.C_raw, dtype=np.float32).copy(),
                   b0_new=np.array(s.b0_new, dtype=np.float64))
        for n, idx in enumerate(video.owned):
            out["W%d" % n] = s.get_W(idx)[::7].data.copy()    # every seventh row of W
        eng.synchronize()
        return out, {c: eng.counter(c) for c in COUNTERS}
    finally:
        eng.close()


_REF = {}


def _pair(te, key, **kw):
    """(reference with temporal_early = 0 -- computed once per configuration and shared --, run with temporal_early = te, its counters); asserts equal outputs"""
    if key not in _REF:
        _REF[key] = _run(0, **kw)
    (ref, cref), (got, cnt) = _REF[key], _run(te, **kw)
    assert cref == dict.fromkeys(COUNTERS, 0), cref          # (temporal_early = 0: today's path, nothing counted)
    assert ref.keys() == got.keys()
    for name in ref:
        assert np.all(np.isfinite(ref[name])), name
        assert ref[name].shape == got[name].shape, name
        assert np.array_equal(ref[name], got[name]), (key, name, float(np.abs(ref[name].astype(np.float64) - got[name].astype(np.float64)).max()))
    return ref, got, cnt


POSITIVE = [
    ("tiny hals", {}, {}),
    ("tiny fp64 tiled projection", {}, {"proj_i8": 0}),
    ("tiny four digit planes", {}, {"proj_i8_planes": 4}),
    ("tiny hals_thresh", {"spatial_algorithm": "hals_thresh"}, {}),
    ("tiny nnls", {"spatial_algorithm": "nnls"}, {}),
]


@pytest.mark.parametrize("name,okw,opts", POSITIVE, ids=[c[0] for c in POSITIVE])
def test_early_projection_serves_both_iterations(name, okw, opts):
    _, _, cnt = _pair(1, name, opt_kw=okw, opts=opts, **TINY)
    assert cnt["temporal_early_hits"] == 2 and cnt["temporal_early_drops"] == 0 and cnt["temporal_early_declined"] == 0, cnt
    assert cnt["temporal_nowait"] == 2, cnt


def test_each_half_alone():
    """temporal_early = 2: the projection only -- the wait in front of the levels is KEPT, with a footprint term pending (A_prev has neurons): the wait path
    still gives equal values; temporal_early = 3: the levels only"""
    _, _, c2 = _pair(2, "tiny hals", opt_kw={}, opts={}, **TINY)
    assert c2["temporal_early_hits"] == 2 and c2["temporal_nowait"] == 0, c2
    _, _, c3 = _pair(3, "tiny hals", opt_kw={}, opts={}, **TINY)
    assert c3["temporal_early_hits"] == 0 and c3["temporal_early_drops"] == 0 and c3["temporal_nowait"] == 2, c3


@pytest.mark.parametrize("dag", [0, 1])
@pytest.mark.parametrize("maxIter", [1, 5])
def test_levels_without_the_wait(dag, maxIter):
    _, _, cnt = _pair(1, "tiny dag%d it%d" % (dag, maxIter), opt_kw={"maxIter": maxIter}, opts={"sweep_dag": dag}, **TINY)
    assert cnt["temporal_nowait"] == 2 and cnt["temporal_early_hits"] == 2, cnt


def test_neuron_emptied_by_the_spatial_update():
    """ind.size < K: the early projection was queued for a result with an all-zero column -- it is dropped, never claimed"""
    kw = dict(dims=(48, 48), pdims=None, T=300, K=6, r=8, seed=5, fkw=dict(gSig=2.0, gSiz=9, min_sep=8), make=_spurious,
              opt_kw={"spatial_algorithm": "hals_thresh", "maxIter": 3})
    ref, _, cnt = _pair(1, "emptied", **kw)
    assert ref["A"].shape[1] == 7 and not ref["A"][:, 6].any() and ref["A"][:, :6].any(axis=0).all()
    assert cnt["temporal_early_hits"] == 0 and cnt["temporal_early_drops"] >= 1, cnt


def test_more_than_64_masks_over_one_block():
    """70 neurons on a 48 x 48 field (3 x 3 blocks) with a ring of radius 15: every mask grown by the ring reaches the central 16 x 16 block.  The early lists ARE
    the lists of the spatial update's own table (masks grown by the ring), so the limit of 64 binds there first: the spatial update realises the residual, and
    the early request is declined for want of a virtual one before vproj_temporal is asked -- its own decline cannot be made to bind alone.  Either way the
    update projects as before.  (On a 64 x 64 field the same 70 leave 60 over the fullest block and the early path serves it.)"""
    kw = dict(dims=(48, 48), pdims=None, T=300, K=70, r=15, seed=11, fkw=dict(gSig=1.5, gSiz=7, min_sep=3), opt_kw={"maxIter": 2})
    _, _, cnt = _pair(1, "crowded", **kw)
    assert cnt["temporal_early_hits"] == 0 and cnt["temporal_early_declined"] >= 1, cnt


@pytest.mark.parametrize("lanes", [1, 2])
def test_several_patches_are_left_alone(lanes):
    """c4tiny: 2 x 2 patches of 48 x 48 -- the hand-over is for the one-patch field of view; nothing is queued ahead"""
    kw = dict(TINY, pdims=[48, 48])
    _, _, cnt = _pair(1, "c4tiny lanes %d" % lanes, lanes=lanes, **kw)
    assert cnt["temporal_early_hits"] == 0 and cnt["temporal_early_drops"] == 0 and cnt["temporal_early_declined"] == 0, cnt


def test_bg_ssub_is_left_alone():
    _, _, cnt = _pair(1, "tiny bg_ssub 2", opt_kw={"bg_ssub": 2}, **TINY)
    assert cnt["temporal_early_hits"] == 0 and cnt["temporal_early_drops"] == 0, cnt


def test_stale_tag_is_rejected():
    """K changes between the spatial and the temporal update of the second iteration (obj.delete), and the caller claims the early result all the same: the tag
    (K among its fields) rejects it"""
    claimed = []
    def between(s, eng, it):
        if it == 1:
            early = getattr(s, "_early_u", None)
            s.delete([3])
            if isinstance(early, tuple):                     # (temporal_early = 0: nothing was queued, nothing to claim)
                eng.temporal_early_claim(early[0]); claimed.append(early[0])
    _, got, cnt = _pair(1, "tiny delete", between=between, **TINY)
    assert got["A"].shape[1] == TINY["K"] - 1
    assert claimed and cnt["temporal_early_hits"] == 1 and cnt["temporal_early_drops"] == 1, (claimed, cnt)


def test_column_of_stored_zeros():
    """a column whose stored values are all zero: aa = 0 and the host's test says "not updated" -- the neuron is skipped, on the device as on the host"""
    from cnmf_e_amd.engine import Engine
    from cnmf_e_amd.sources2d import PatchedVideo, Sources2D, Options
    dims, T, K, r = (48, 48), 300, 6, 8
    f, Y, A0, C0 = _factors(dims, T, K, 5, dict(gSig=2.0, gSiz=9, min_sep=8))
    res = {}
    for te in (0, 1):
        eng = Engine(0)
        try:
            eng.set_option("temporal_early", te)
            video = PatchedVideo(dims[0], dims[1], T, list(dims), r, eng)
            video.upload_from_full(Y)
            s = Sources2D(video, Options(ring_radius=r, spatial_algorithm="hals", maxIter=3), A0, C0, f.sn)
            s.update_background_parallel(); s.update_spatial_parallel(); s.update_temporal_parallel()
            A = sp.csc_matrix(s.A, dtype=np.float32, copy=True); A.sort_indices()
            A.data[A.indptr[2]:A.indptr[3]] = 0.0                # column 2: its pattern stays, its values are stored zeros
            idx = video.owned[0]
            Cin = np.asarray(s.C, dtype=np.float32).copy()
            Cout, Craw, aa = eng.hals_temporal(video.pid[idx], A, Cin, 3)
            eng.synchronize()
            res[te] = (Cout, Craw, aa, eng.counter("temporal_nowait"))
        finally:
            eng.close()
    (C0_, R0, a0, n0), (C1, R1, a1, n1) = res[0], res[1]
    assert n0 == 0 and n1 == 2, (n0, n1)
    assert a0[2] == 0.0 and a1[2] == 0.0 and np.array_equal(a0, a1)
    assert np.array_equal(C0_, C1) and np.array_equal(R0, R1)
    assert np.array_equal(C1[2], Cin[2]) and not R1[2].any()     # HALS_temporal.m:51: the row is left alone, C_raw(k,:) stays 0
