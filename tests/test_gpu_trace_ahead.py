"""Option ring_side (resid.hip, ring_side_ahead; common.hpp, SideScope::fork_behind): a ring fit records an event right behind its solve and queues, on the context's side stream behind
that event, the statistics of the new W (k_ring_pmax, the row-1 copy) and the W*A tables of the residual request that follows the fit; the request takes them when
its A is the fit's.  The device then runs them beside the spatial update's kernels.  2 joins at once (the same streams and code, nothing concurrent: a wrong
stream shows in 1 and 2, a hazard of the overlap in 1 only).  Only WHEN and WHERE the kernels run changes, so every run here must give, under np.array_equal, what
the same calls give with ring_side = 0 (one stream): A, C, b0_new and sampled rows of W after every background update.

(The file keeps the name the issue gave it; the issue's other half, option trace_ahead, was measured and is not in the tree: profiles/trace_ahead/README.md.)

Shapes: 96 x 96, K = 18, T = 2304 with ring radius 15 (the int8 window path with three digit planes), 48 x 48, T = 608 with radius 5, and 40 x 36, T = 9200 with
radius 5 for the frame stride 2.  The reference run of a case is computed once and shared by the modes."""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

BIG = dict(dims=(96, 96), T=2304, K=18, r=15)
SMALL = dict(dims=(48, 48), T=608, K=8, r=5)
NROWS, ROW_SEED, SEED = 24, 20262, 23

_REF = {}                                                    # case -> arrays under ring_side = 0


def _bits(x):
    return np.ascontiguousarray(x, dtype=np.float32).view(np.uint32)


def _rows(d, n=NROWS):
    return np.sort(np.random.default_rng(ROW_SEED).choice(d, size=min(n, d), replace=False))


def _snapshot(out, tag, s, video, W_too=True):
    A = s.A.tocsc(); A.sort_indices()
    out[tag + "_A_indptr"], out[tag + "_A_indices"], out[tag + "_A"] = A.indptr.astype(np.int64), A.indices.astype(np.int64), _bits(A.data)
    out[tag + "_C"] = _bits(np.asarray(s.C, dtype=np.float32))
    out[tag + "_b0_new"] = np.ascontiguousarray(np.asarray(s.b0_new, dtype=np.float64)).view(np.uint64)
    if W_too:
        for n, idx in enumerate(video.owned):
            W = s.get_W(idx).tocsr()
            out["%s_W%d" % (tag, n)] = _bits(W[_rows(W.shape[0])].data)
            assert np.all(np.isfinite(W.data))


def run(mode, dims, T, K, r, script, pdims=None, lanes=1, okw=None, opts=None):
    """script(s, video, eng, out, f): the calls of the case.  -> arrays"""
    from cnmf_e_amd import synth
    from cnmf_e_amd.engine import Engine
    from cnmf_e_amd.sources2d import PatchedVideo, Sources2D, Options
    f = synth.make_factors(dims[0], dims[1], T, K, SEED, gSig=2.0, gSiz=9, min_sep=5)
    Y = synth.make_video(f, np.float32)
    eng = Engine(0)
    out = {}
    try:
        if lanes > 1:
            eng.set_option("lanes", lanes)
        eng.set_option("ring_side", mode)
        for k, v in (opts or {}).items():
            eng.set_option(k, v)
        video = PatchedVideo(dims[0], dims[1], T, pdims or list(dims), r, eng)
        video.upload_from_full(Y)
        kw = dict(spatial_algorithm="hals", maxIter=3); kw.update(okw or {})
        s = Sources2D(video, Options(ring_radius=r, **kw), f.A_init, f.C_init, f.sn)
        script(s, video, eng, out, f)
        eng.synchronize()
    finally:
        eng.close()
    return out


def _iteration(s, video, out, tag, **spatial_kw):
    info = s.update_background_parallel()
    _snapshot(out, tag + "_bg", s, video)
    s.update_spatial_parallel(**spatial_kw)
    s.update_temporal_parallel()
    _snapshot(out, tag, s, video, W_too=False)
    return info


def _same(name, mode, ref, got):
    assert ref.keys() == got.keys(), (name, mode, sorted(set(ref) ^ set(got)))
    for k in ref:
        assert ref[k].shape == got[k].shape and ref[k].dtype == got[k].dtype, (name, mode, k, ref[k].shape, got[k].shape)
        assert np.array_equal(ref[k], got[k]), (name, mode, k, int((ref[k] != got[k]).sum()), ref[k].size)


# ---- the cases --------------------------------------------------------------------------------------------------------------------------------------------------
def three_iterations(s, video, eng, out, f):
    for it in range(3):
        _iteration(s, video, out, "it%d" % it)


def rebind_between(s, video, eng, out, f):
    """the traces and the footprints are replaced between the temporal update and the fit"""
    _iteration(s, video, out, "it0")
    _iteration(s, video, out, "it1")
    C2 = np.ascontiguousarray(np.asarray(s.C, dtype=np.float32) * np.float32(1.25) + np.float32(0.5))
    s.set_components(s.A, C2)
    _iteration(s, video, out, "it2")
    _iteration(s, video, out, "it3")


def delete_between(s, video, eng, out, f):
    """a neuron goes between the updates, once between the spatial and the temporal update: that temporal update's request names another A than the fit's, so
    the tables built behind the solve must not be taken"""
    _iteration(s, video, out, "it0")
    _iteration(s, video, out, "it1")
    s.delete([2])
    _iteration(s, video, out, "it2")
    s.update_spatial_parallel()
    s.delete([0])
    s.update_temporal_parallel()
    _iteration(s, video, out, "it3")


def two_temporal(s, video, eng, out, f):
    """two temporal updates in a row with no fit between them: a term pends across a stitch, C_prev is older than the bound matrix"""
    _iteration(s, video, out, "it0")
    _iteration(s, video, out, "it1")
    s.update_temporal_parallel()
    _snapshot(out, "t2", s, video, W_too=False)
    s.update_spatial_parallel()
    s.update_temporal_parallel()
    s.update_temporal_parallel()
    _snapshot(out, "t3", s, video, W_too=False)
    _iteration(s, video, out, "it2")


def with_noise_and_rss(s, video, eng, out, f):
    """consumers that realise the residual: update_sn in the spatial call, compute_RSS right behind an iteration"""
    _iteration(s, video, out, "it0")
    _iteration(s, video, out, "it1", update_sn=True)
    total, _ = s.compute_RSS()
    out["rss1"] = np.array([total], dtype=np.float64).view(np.uint64)
    _iteration(s, video, out, "it2", update_sn=True)
    total, _ = s.compute_RSS()
    out["rss2"] = np.array([total], dtype=np.float64).view(np.uint64)
    _iteration(s, video, out, "it3")


def strided(s, video, eng, out, f):
    """T = 9200 at radius 5: fit_stride gives 2 (tests/test_gpu_packed.py has this geometry), the strided fit with the fp32 window kernel"""
    strides = [int(next(iter(_iteration(s, video, out, "it%d" % it).values()))["frame_stride"]) for it in range(3)]
    out["strides"] = np.array(strides, dtype=np.int64)
    assert 2 in strides, strides


CASES = {
    "three_iterations_r15": (BIG, three_iterations, {}),
    "three_iterations_r5": (SMALL, three_iterations, {}),
    "rebind_r15": (BIG, rebind_between, {}),
    "rebind_r5": (SMALL, rebind_between, {}),
    "delete_r15": (BIG, delete_between, {}),
    "delete_r5": (SMALL, delete_between, {}),
    "two_temporal_r15": (BIG, two_temporal, {}),
    "two_temporal_r5": (SMALL, two_temporal, {}),
    "deconv_r5": (SMALL, three_iterations, dict(okw={"deconv_flag": True})),
    "stride2": (dict(dims=(40, 36), T=9200, K=5, r=5), strided, {}),
    "noise_rss_r15": (BIG, with_noise_and_rss, {}),
    "noise_rss_r5": (SMALL, with_noise_and_rss, {}),
    # four patches on one lane: more than one patch in the context, the mechanism is inert
    "patches_one_lane": (dict(dims=(96, 96), T=608, K=18, r=5), three_iterations, dict(pdims=[48, 48])),
    # lanes = 2: the mechanism is inert
    "patches_two_lanes": (dict(dims=(96, 96), T=608, K=18, r=5), three_iterations, dict(pdims=[48, 48], lanes=2)),
    # the swept residual (no virtual request): the ring sweep reads the traces of the call, the term is applied, not pending
    "swept_r5": (SMALL, three_iterations, dict(opts={"r1_virtual": 0})),
}


def _run_case(name, mode):
    shape, script, kw = CASES[name]
    return run(mode, script=script, **shape, **kw)


PARAMS = [(n, m) for n in CASES for m in (1, 2)]


@pytest.mark.gpu
@pytest.mark.parametrize("name,mode", PARAMS, ids=["%s-rs%d" % (n, m) for n, m in PARAMS])
def test_same_bits_as_without_the_options(name, mode):
    if name not in _REF:
        _REF[name] = _run_case(name, 0)
    _same(name, mode, _REF[name], _run_case(name, mode))


@pytest.mark.gpu
def test_profile_names_and_one_table_build_per_iteration():
    """in profile mode the side kernels are reported by their names (their events lie on the side stream), and the steady-state iteration builds the W*A tables
    once: the fit builds them, the temporal update's request takes them"""
    counts = {}

    def script(s, video, eng, out, f):
        eng.profile(True)
        _iteration(s, video, out, "it0")
        for it in (1, 2):
            eng.profile_reset()
            _iteration(s, video, out, "it%d" % it)
            eng.synchronize()
            counts[(eng.get_option("ring_side", 1), it)] = {n: v["calls"] for n, v in eng.profile_table().items() if v["calls"] > 0}
        eng.profile(False)

    outs = {m: run(m, script=script, **BIG) for m in (0, 1, 2)}
    for m in (1, 2):
        _same("profiled", m, outs[0], outs[m])
    for it in (1, 2):
        for m in (0, 1, 2):
            c = counts[(m, it)]
            assert c.get("ring_pmax") == 1 and c.get("r1_ring_wa") == 1, (m, it, c)
            assert c.get("center_traces") == 3 and c.get("bg_trace_dig") == 1 and c.get("bg_trace_gram") == 1, (m, it, c)
