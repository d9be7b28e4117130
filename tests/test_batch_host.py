"""Batch mode on the CPU (cnmf_e_amd/batch.py): the frame-range rule against cases worked by hand, and the parent object's own logic -- the weighted footprint
average, the empty-column rule, spread_all, the refusals, the order of calls of initComponents_batch -- against an engine double.

The double subclasses tests/fake_engine.py::FakeEngine (float64 oracle kernels) and adds what batch mode asks of an engine: trace_energy (numpy, float64),
traces_grow with the bookkeeping of Engine.traces_grow, and a call log.  The single-recording methods whose numerics are not the subject here
(initComponents_parallel, initTemporal, the updates) are replaced per object by recorders that leave a prescribed state; their own tests are elsewhere."""
import os
import sys

import numpy as np
import pytest
import scipy.sparse as sp

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for p in (HERE, os.path.join(ROOT, "oracle")):
    if p not in sys.path:
        sys.path.insert(0, p)

import batch_cases as bc


@pytest.fixture(scope="module")
def built():
    if not os.path.exists(os.path.join(ROOT, "cnmf_e_amd", "libcnmfe_hip.so")):
        import cnmf_e_amd.build as b
        b.build(verbose=False)
    return True


def test_frame_ranges_by_hand(built):
    from cnmf_e_amd.batch import batch_frame_ranges
    for (T, bf), want in bc.frame_ranges_by_hand().items():
        assert batch_frame_ranges(T, bf) == want, (T, bf)
    assert round(100 / 40) == 2                                  # what Python's round would have made of the second case
    # every frame belongs to exactly one range
    for T, bf in ((1000, 300), (100, 40), (304, 101), (999, 7)):
        r = batch_frame_ranges(T, bf)
        assert r[0][0] == 1 and r[-1][1] == T and all(r[i][1] + 1 == r[i + 1][0] for i in range(len(r) - 1))


def test_package_exports(built):
    import cnmf_e_amd
    from cnmf_e_amd.batch import Sources2DBatch, batch_frame_ranges
    assert cnmf_e_amd.Sources2DBatch is Sources2DBatch and cnmf_e_amd.batch_frame_ranges is batch_frame_ranges


# ---- the engine double ---------------------------------------------------------------------------------------------------------------------------------------
def _fake_engine_class():
    from fake_engine import FakeEngine

    class BatchFakeEngine(FakeEngine):
        supports_bound_traces = True
        supports_traces_grow = True

        def __init__(self, log, tag):
            super().__init__()
            self.log, self.tag = log, tag
            self._bound = None

        def bind_traces(self, Cm):
            self._bound = None if Cm is None or Cm.shape[0] == 0 else Cm
            self.log.append((self.tag, "bind", None if self._bound is None else self._bound.shape))

        def ring_csr(self, pid):
            self.log.append((self.tag, "ring_csr", pid))
            return super().ring_csr(pid)

        def trace_energy(self, X):
            self.log.append((self.tag, "trace_energy", "bound" if X is self._bound else "host"))
            return (np.asarray(X, dtype=np.float64) ** 2).sum(axis=1)

        def traces_grow(self, K_new):
            from cnmf_e_amd.engine import GrownTraces
            self.log.append((self.tag, "traces_grow", int(K_new)))
            assert self._bound is not None and K_new >= self._bound.shape[0]
            if K_new > self._bound.shape[0]:
                self._bound = GrownTraces(self._bound, K_new)
            return self._bound, None, None

        def residents_are(self, Cm, C_raw, S):
            return False
    return BatchFakeEngine


def _col(pix, val, d):
    return sp.csc_matrix((np.asarray(val, dtype=np.float32), (np.asarray(pix), np.zeros(len(pix), dtype=np.int64))), shape=(d, 1))


def _batches(frames=(64, 70, 66), pdims=(16, 16), K=0, ring=3, dist=None, d1=16, d2=16):
    """fresh Sources2D objects on engine doubles (zero videos: nothing here reads them), a shared call log"""
    from cnmf_e_amd.sources2d import PatchedVideo, Sources2D, Options
    Eng = _fake_engine_class()
    log, out = [], []
    d = d1 * d2
    for m, n in enumerate(frames):
        eng = Eng(log, m)
        video = PatchedVideo(d1, d2, n, list(pdims), ring, eng)
        out.append(Sources2D(video, Options(ring_radius=ring), sp.csc_matrix((d, K), dtype=np.float32), np.zeros((K, n), np.float32), np.ones(d, np.float32), dist_group=dist))
    return out, log


def test_refusals(built):
    from cnmf_e_amd.batch import Sources2DBatch
    from cnmf_e_amd.sources2d import Options
    ok, _ = _batches()
    b = Sources2DBatch(ok, Options(ring_radius=3))
    assert all(s.options is b.options for s in b.batches)                     # ONE options object (initComponents_batch.m:40,92)
    assert b.P["numFrames"].tolist() == [64, 70, 66] and b.file_id.tolist() == [1, 1, 1] and b.A.shape == (256, 0) and b.P["k_ids"] == 0
    with pytest.raises(ValueError):                                           # another field of view
        Sources2DBatch(_batches()[0][:1] + _batches(d1=20)[0][:1], Options(ring_radius=3))
    with pytest.raises(ValueError):                                           # other patches
        Sources2DBatch(_batches(d1=32, d2=32, pdims=(32, 32))[0][:1] + _batches(d1=32, d2=32, pdims=(16, 16))[0][:1], Options(ring_radius=3))
    with pytest.raises(ValueError):                                           # another ring radius
        Sources2DBatch(_batches()[0][:1] + _batches(ring=4)[0][:1], Options(ring_radius=3))
    with pytest.raises(ValueError):                                           # ... also when only the shared options disagree
        Sources2DBatch(_batches()[0], Options(ring_radius=4))
    with pytest.raises(ValueError):                                           # fewer than 64 frames
        Sources2DBatch(_batches(frames=(64, 63))[0], Options(ring_radius=3))
    with pytest.raises(ValueError):                                           # a sharded batch
        Sources2DBatch(_batches(dist=object())[0], Options(ring_radius=3))
    two, _ = _batches()
    two[1].engine = two[0].engine
    with pytest.raises(ValueError):                                           # one context for two batches
        Sources2DBatch(two, Options(ring_radius=3))
    with pytest.raises(NotImplementedError):
        b.initComponents_batch(save_avi=True)


def _stub_spatial(s, A_new):
    def upd(*a, **k):
        s.engine.log.append((s.engine.tag, "update_spatial_parallel", None))
        s.A = A_new
    s.update_spatial_parallel = upd


def test_weighted_average_empty_column_spread(built):
    from cnmf_e_amd.batch import Sources2DBatch
    from cnmf_e_amd.sources2d import Options
    rng = np.random.default_rng(3)
    d, K = 256, 4
    for spread_all in (False, True):
        bs, log = _batches(K=K)
        A_k, C_k = [], []
        for m, s in enumerate(bs):
            A = sp.random(d, K, density=0.05, random_state=10 + m, format="csc", dtype=np.float32)
            C = rng.uniform(0.0, 3.0, (K, s.video.T)).astype(np.float32)
            C[2] = 0.0                                                         # neuron 2 has no energy in any batch
            if m == 1:
                C[0] = 0.0                                                     # neuron 0 none in batch 2 alone: that batch's footprint does not count
                A = sp.csc_matrix(np.where(np.arange(K)[None, :] == 0, np.nan, A.toarray()).astype(np.float32))      # ... whatever its update left (0 * NaN)
            s.set_components(sp.csc_matrix((d, K), dtype=np.float32), C)
            _stub_spatial(s, A)
            A_k.append(A); C_k.append(C)
        b = Sources2DBatch(bs, Options(ring_radius=3))
        b.A = sp.csc_matrix((d, K), dtype=np.float32)
        del log[:]
        dead = b.update_spatial_batch(spread_all=spread_all)
        want, dead_want = bc.weighted_average(A_k, C_k)
        assert dead.tolist() == dead_want.tolist() == [2]
        got = b.A.toarray()
        assert b.A.dtype == np.float32 and np.isfinite(got).all() and bc.within_one_ulp(got, want)
        assert b.A.indptr[3] == b.A.indptr[2]                                  # an EMPTY column, not stored zeros
        holds_avg = [np.array_equal(s.A.toarray(), got) for s in bs]
        assert holds_avg == ([True, True, True] if spread_all else [True, True, False])
        if not spread_all:
            assert np.array_equal(bs[-1].A.toarray(), A_k[-1].toarray(), equal_nan=True)      # the last batch keeps its own update (update_spatial_batch.m:37)
        # per batch: the update, then the weights where the traces lie; nothing is bound again by handing A down
        assert [e[1] for e in log] == ["update_spatial_parallel", "trace_energy"] * 3 and all(e[2] in (None, "bound") for e in log)
    bs, _ = _batches()
    assert Sources2DBatch(bs, Options(ring_radius=3)).update_spatial_batch().size == 0       # K = 0: "You have to initialize neurons first"


def test_init_components_batch_call_order(built):
    """batch 1 finds 2 neurons and 1 more in its residual; batch 2 none; batch 3 finds a fourth: batches 1 and 2 grow to 4 and update their traces"""
    from cnmf_e_amd.batch import Sources2DBatch
    from cnmf_e_amd.sources2d import Options
    bs, log = _batches()
    d = 256
    found = {0: 1, 1: 0, 2: 1}

    def rec(s, name):
        s.engine.log.append((s.engine.tag, name, s.A.shape[1]))

    for m, s in enumerate(bs):
        def init_par(K=None, s=s):
            rec(s, "initComponents_parallel")
            s.set_components(sp.hstack([_col([5, 6], [1, 2], d), _col([40], [3], d)], format="csc"), np.ones((2, s.video.T), np.float32))
            s.S = np.zeros_like(s.C)
            s.ids = np.arange(1, 3); s.tags = np.zeros(2, np.uint16); s.P["k_ids"] = 2

        def init_temp(s=s):
            rec(s, "initTemporal")
            assert s.engine.ring_first_run(s.video.pid[(0, 0)])               # nothing was transplanted: the ring still says "first run"
            s.C = s.C_raw = np.full((s.A.shape[1], s.video.T), 2.0, np.float32)
            s._bind_C()

        def upd_bg(s=s):
            rec(s, "update_background_parallel")

        def init_res(s=s, m=m):
            rec(s, "initComponents_residual_parallel")
            n = found[m]
            if n:
                K0 = s.A.shape[1]
                s.set_components(sp.hstack([s.A, _col([100 + m], [1], d)], format="csc"), np.concatenate([np.asarray(s.C), np.full((n, s.video.T), 7.0, np.float32)]))
                s.ids = np.concatenate([s.ids, s.P["k_ids"] + np.arange(1, n + 1)]); s.tags = np.concatenate([s.tags, np.zeros(n, np.uint16)]); s.P["k_ids"] += n
                if getattr(s, "S", None) is not None:
                    s.S = np.zeros_like(np.asarray(s.C))
                assert s.A.shape[1] == K0 + n

        def upd_t(s=s):
            rec(s, "update_temporal_parallel")
            assert s.C.shape[0] == s.A.shape[1] == 4 and s.engine._bound is s.C

        s.initComponents_parallel, s.initTemporal, s.update_background_parallel = init_par, init_temp, upd_bg
        s.initComponents_residual_parallel, s.update_temporal_parallel = init_res, upd_t
    b = Sources2DBatch(bs, Options(ring_radius=3))
    del log[:]
    b.initComponents_batch(K=7)
    methods = [(t, n, k) for (t, n, k) in log if n not in ("bind", "ring_csr", "traces_grow")]
    assert methods == [
        (0, "initComponents_parallel", 0), (0, "update_background_parallel", 2), (0, "initComponents_residual_parallel", 2),
        (1, "initTemporal", 3), (1, "update_background_parallel", 3), (1, "initComponents_residual_parallel", 3),
        (2, "initTemporal", 3), (2, "update_background_parallel", 3), (2, "initComponents_residual_parallel", 3),
        (0, "update_temporal_parallel", 4), (1, "update_temporal_parallel", 4)], methods      # batch 3 is complete: no temporal update (:94-96)
    names = [(t, n) for (t, n, _) in log]
    # W of batch 1 is read once, after its greedy pass and before its first fit; every later batch's before its initTemporal
    i_w0 = names.index((0, "ring_csr"))
    assert names.index((0, "initComponents_parallel")) < i_w0 < names.index((0, "update_background_parallel"))
    for m in (1, 2):
        assert names.index((m, "ring_csr")) < names.index((m, "initTemporal"))
    # the growth happens on the engine (no bind between a batch's traces_grow and its temporal update), from 3 rows to 4
    grows = [(t, k) for (t, n, k) in log if n == "traces_grow"]
    assert grows == [(0, 4), (1, 4)]
    for m in (0, 1):
        i = names.index((m, "traces_grow"))
        assert names[i + 1] == (m, "update_temporal_parallel")
    # the parent and every batch: one A, continued ids, same tags
    assert b.A.shape[1] == 4 and b.ids.tolist() == [1, 2, 3, 4] and b.P["k_ids"] == 4
    for s in bs:
        assert s.A.shape[1] == 4 and np.array_equal(s.A.toarray(), b.A.toarray()) and s.ids.tolist() == [1, 2, 3, 4] and s.P["k_ids"] == 4 and len(s.tags) == 4
        assert s.C.shape == (4, s.video.T) and s.options is b.options
    assert np.array_equal(np.asarray(bs[0].C)[3], np.zeros(64, np.float32)) and np.array_equal(np.asarray(bs[0].C)[:3], np.concatenate([np.ones((2, 64)), np.full((1, 64), 7.0)]).astype(np.float32))
    assert bs[0].S.shape == (4, 64)
    # the other loops
    del log[:]
    b.update_temporal_batch(); b.update_background_batch()
    assert [(t, n) for (t, n, _) in log if n != "bind"] == [(m, "update_temporal_parallel") for m in range(3)] + [(m, "update_background_parallel") for m in range(3)]
    b.concatenate_temporal_batch()
    assert b.C.shape == b.C_raw.shape == (4, 200) and b.C.dtype == np.float32 and b.S is None
    assert np.array_equal(b.C[:, 64:134], np.asarray(bs[1].C)) and np.array_equal(b.C_raw[:, 134:], np.asarray(bs[2].C_raw))


def test_a_transplanted_ring_is_refused(built):
    from cnmf_e_amd.batch import Sources2DBatch
    from cnmf_e_amd.sources2d import Options
    bs, _ = _batches()
    for s in bs:
        s.initComponents_parallel = lambda K=None, s=s: (s.set_components(_col([5], [1], 256), np.ones((1, s.video.T), np.float32)),
                                                          setattr(s, "ids", np.arange(1, 2)), setattr(s, "tags", np.zeros(1, np.uint16)), s.P.__setitem__("k_ids", 1))
        s.update_background_parallel = lambda: None
        s.initComponents_residual_parallel = lambda: None
    W = bs[1].engine.p[0]["W"].copy(); W.data = W.data * 0.5
    bs[1].engine.p[0]["W"] = W                                                 # batch 2 does not come fresh
    with pytest.raises(RuntimeError):
        Sources2DBatch(bs, Options(ring_radius=3)).initComponents_batch()


def test_grow_K_host_path(built):
    """an engine without traces_grow: padded on the host, bound again"""
    from cnmf_e_amd.sources2d import Options
    bs, log = _batches(K=2)
    s = bs[0]
    type(s.engine).supports_traces_grow = False
    try:
        s.set_components(s.A, np.ones((2, 64), np.float32), np.full((2, 64), 2.0, np.float32))
        s.S = np.full((2, 64), 3.0, np.float32); s.P["kernel_pars"] = np.array([0.5, 0.6]); s.P["neuron_sn"] = np.array([1.0, 1.0], np.float32)
        with pytest.raises(ValueError):
            s._grow_K(1)
        with pytest.raises(ValueError):
            s._grow_K(3)                                                       # obj.A comes first
        s._set_A(sp.hstack([s.A, _col([9], [1], 256)], format="csc"))
        del log[:]
        s._grow_K(3)
        assert [e[1] for e in log] == ["bind"] and s.engine._bound is s.C
        for X, v in ((s.C, 1.0), (s.C_raw, 2.0), (s.S, 3.0)):
            assert X.shape == (3, 64) and np.all(np.asarray(X)[:2] == v) and np.all(np.asarray(X)[2] == 0)
        assert s.P["kernel_pars"].tolist() == [0.5, 0.6, 0.0] and s.P["neuron_sn"].tolist() == [1.0, 1.0, 0.0]
        s._grow_K(3)                                                           # nothing to do
        assert [e[1] for e in log] == ["bind"]
    finally:
        type(s.engine).supports_traces_grow = True


def test_grow_fixture(built):
    """the condition on the fixture of tests/test_gpu_batch.py::test_K_grows_across_batches, on the CPU (tests/batch_cases.py: GROW)"""
    got = bc.grow_oracle_check()
    print("grow fixture:", got)
    assert got["nearest_batch1"] > 3                                           # batch 1's search does not find the late neuron
    assert got["found"] is not None                                            # batch 2's residual search does ...
    assert got["cn_pnr"] >= 1.5 * got["threshold"]                             # ... with margin
    assert got["footprint_corr"] > 0.9                                         # the footprint the search extracts is the neuron's (the GPU test asks for 0.8)
    assert got["seed_pixels"] >= 10                                            # (greedyROI_endoscope starts a search with K = numel(seeds) / 10 >= 1 only)
    rec = bc.GROW_RECORDED
    assert tuple(got["centre"]) == tuple(rec["centre"]) and tuple(got["found"]) == tuple(rec["found"]) and got["seed_pixels"] == rec["seed_pixels"]
    assert abs(got["cn_pnr"] - rec["cn_pnr"]) < 0.01 and abs(got["nearest_batch1"] - rec["nearest_batch1"]) < 0.1 and got["threshold"] == rec["threshold"] and abs(got["footprint_corr"] - rec["footprint_corr"]) < 0.001
