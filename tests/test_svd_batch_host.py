"""Batch mode under background_model = 'svd' on the CPU (cnmf_e_amd/batch.py): the order of calls of initComponents_batch, the hand-down of the spatial background
from batch to batch (set_bg_svd with the previous batch's b and zeros of the receiving batch's shapes), and the refusal of engines that do not declare
supports_bg_svd_init_temporal.  The engine double composes tests/svd_fake_engine.py::SvdFakeEngine with the few calls batch mode adds (as tests/test_batch_host.py
does for the ring model); the single-recording methods are replaced per object by recorders that leave a prescribed state -- their numerics are tested elsewhere."""
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

NB = 2


def _engine_class(flag=True):
    from svd_fake_engine import SvdFakeEngine

    class SvdBatchFakeEngine(SvdFakeEngine):
        supports_bound_traces = True
        supports_traces_grow = True
        supports_bg_svd_init_temporal = flag

        def __init__(self, log, tag):
            super().__init__()
            self.log, self.tag = log, tag
            self._bound = None

        def bind_traces(self, Cm):
            self._bound = None if Cm is None or Cm.shape[0] == 0 else Cm

        def bg_svd_set(self, pid, b, f, b0):
            self.log.append((self.tag, "bg_svd_set", pid))
            return super().bg_svd_set(pid, b, f, b0)

        def traces_grow(self, K_new):
            from cnmf_e_amd.engine import GrownTraces
            self.log.append((self.tag, "traces_grow", int(K_new)))
            if K_new > self._bound.shape[0]:
                self._bound = GrownTraces(self._bound, K_new)
            return self._bound, None, None

        def residents_are(self, Cm, C_raw, S):
            return False
    return SvdBatchFakeEngine


def _col(pix, val, d):
    return sp.csc_matrix((np.asarray(val, dtype=np.float32), (np.asarray(pix), np.zeros(len(pix), dtype=np.int64))), shape=(d, 1))


def _batches(frames=(64, 70, 66), flag=True, model="svd"):
    """fresh Sources2D objects of a 32 x 32 field in 2 x 2 patches on engine doubles (zero videos: nothing here reads them), a shared call log"""
    from cnmf_e_amd.sources2d import PatchedVideo, Sources2D, Options
    Eng = _engine_class(flag)
    log, out = [], []
    d = 32 * 32
    for m, n in enumerate(frames):
        eng = Eng(log, m)
        video = PatchedVideo(32, 32, n, [16, 16], 3, eng)
        out.append(Sources2D(video, Options(ring_radius=3, background_model=model, nb=NB), sp.csc_matrix((d, 0), dtype=np.float32), np.zeros((0, n), np.float32),
                             np.ones(d, np.float32)))
    return out, log


def test_engine_flag_and_refusals():
    from cnmf_e_amd.batch import Sources2DBatch
    from cnmf_e_amd.engine import Engine
    from cnmf_e_amd.sources2d import Options
    assert Engine.supports_bg_svd_init_temporal is True
    opt = Options(ring_radius=3, background_model="svd", nb=NB)
    ok, _ = _batches()
    b = Sources2DBatch(ok, opt)
    assert b.svd and all(s.options is opt for s in b.batches)
    with pytest.raises(NotImplementedError, match="supports_bg_svd_init_temporal"):      # an engine without the flag
        Sources2DBatch(_batches(flag=False)[0], opt)
    with pytest.raises(NotImplementedError, match="supports_bg_svd_init_temporal"):      # ... even one
        Sources2DBatch(_batches()[0][:2] + _batches(flag=False)[0][:1], opt)
    with pytest.raises(ValueError):                                                      # the model is the shared options' AND every batch's
        Sources2DBatch(_batches()[0], Options(ring_radius=3))
    with pytest.raises(ValueError):
        Sources2DBatch(_batches()[0][:1] + _batches(model="ring")[0][:1], opt)
    # the single-recording method keeps its refusal for an engine without the flag
    s = _batches(flag=False)[0][0]
    s.A = _col([5], [1.0], 32 * 32)
    with pytest.raises(NotImplementedError, match="svd"):
        s.initTemporal()


def test_init_components_batch_order_and_hand_down():
    """batch 1 finds 2 neurons and a third in its second pass; batch 2 none; batch 3 a fourth.  Every batch after the first receives, per patch and BEFORE its
    initTemporal, the b the batch before it held AFTER its background update and second pass, with f = zeros((nb, T_k)) and b0 = zeros(d_patch); no ring is read."""
    from cnmf_e_amd.batch import Sources2DBatch
    from cnmf_e_amd.sources2d import Options
    bs, log = _batches()
    d = 32 * 32
    found = {0: 1, 1: 0, 2: 1}
    seen = {}

    def rec(s, name):
        s.engine.log.append((s.engine.tag, name, s.A.shape[1]))

    def b_of(m, idx, n, stage):
        return np.full((n, NB), 10.0 * (m + 1) + idx[0] + 0.1 * idx[1] + stage)

    for m, s in enumerate(bs):
        def init_par(K=None, s=s):
            rec(s, "initComponents_parallel")
            s.set_components(sp.hstack([_col([5, 6], [1, 2], d), _col([700], [3], d)], format="csc"), np.ones((2, s.video.T), np.float32))
            s.ids = np.arange(1, 3); s.tags = np.zeros(2, np.uint16); s.P["k_ids"] = 2

        def init_temp(s=s, m=m):
            rec(s, "initTemporal")
            seen[m] = {idx: (s.get_b(idx), s.get_f(idx), s.get_b0(idx)) for idx in s.video.owned}
            s.C = s.C_raw = np.full((s.A.shape[1], s.video.T), 2.0, np.float32)
            s._bind_C()

        def upd_bg(s=s, m=m):
            rec(s, "update_background_parallel")
            for idx in s.video.owned:                                          # a fit: new b, f, b0
                n = s.video.patch_pix[idx].size
                s.engine.p[s.video.pid[idx]]["svd"] = (b_of(m, idx, n, 0.0), np.ones((NB, s.video.T)), np.ones(n))

        def init_res(s=s, m=m):
            rec(s, "initComponents_residual_parallel")
            for idx in s.video.owned:                                          # (the real second pass leaves b alone; the recorder moves it to show WHEN it is read)
                q = s.engine.p[s.video.pid[idx]]
                q["svd"] = (q["svd"][0] + 0.5,) + q["svd"][1:]
            if found[m]:
                s.set_components(sp.hstack([s.A, _col([100 + m], [1], d)], format="csc"), np.concatenate([np.asarray(s.C), np.full((1, s.video.T), 7.0, np.float32)]))
                s.ids = np.concatenate([s.ids, s.P["k_ids"] + np.arange(1, 2)]); s.tags = np.concatenate([s.tags, np.zeros(1, np.uint16)]); s.P["k_ids"] += 1

        def upd_t(s=s):
            rec(s, "update_temporal_parallel")
            assert s.C.shape[0] == s.A.shape[1] == 4

        s.initComponents_parallel, s.initTemporal, s.update_background_parallel = init_par, init_temp, upd_bg
        s.initComponents_residual_parallel, s.update_temporal_parallel = init_res, upd_t
        s.get_W = lambda idx: pytest.fail("get_W under the svd model")
    b = Sources2DBatch(bs, Options(ring_radius=3, background_model="svd", nb=NB))
    del log[:]
    b.initComponents_batch(K=7)
    methods = [(t, n, k) for (t, n, k) in log if n not in ("bg_svd_set", "traces_grow", "ring_init", "bg_svd_fit", "residual_lowrank")]
    assert methods == [
        (0, "initComponents_parallel", 0), (0, "update_background_parallel", 2), (0, "initComponents_residual_parallel", 2),
        (1, "initTemporal", 3), (1, "update_background_parallel", 3), (1, "initComponents_residual_parallel", 3),
        (2, "initTemporal", 3), (2, "update_background_parallel", 3), (2, "initComponents_residual_parallel", 3),
        (0, "update_temporal_parallel", 4), (1, "update_temporal_parallel", 4)], methods
    names = [(t, n) for (t, n, _) in log]
    npatch = len(bs[0].video.owned)
    assert npatch == 4 and (0, "bg_svd_set") not in names
    for m in (1, 2):
        sets = [i for i, e in enumerate(names) if e == (m, "bg_svd_set")]
        assert len(sets) == npatch and sets[-1] < names.index((m, "initTemporal")) and sets[0] > names.index((m - 1, "initComponents_residual_parallel"))
        assert sorted(log[i][2] for i in sets) == sorted(bs[m].video.pid[idx] for idx in bs[m].video.owned)
        for idx in bs[m].video.owned:
            n = bs[m].video.patch_pix[idx].size
            bb, ff, b00 = seen[m][idx]
            assert np.array_equal(bb, b_of(m - 1, idx, n, 0.5))                # the batch before, after its fit AND its second pass
            assert ff.shape == (NB, bs[m].video.T) and not ff.any() and b00.shape == (n,) and not b00.any()
    assert b.A.shape[1] == 4 and b.ids.tolist() == [1, 2, 3, 4] and b.P["k_ids"] == 4
    for s in bs:
        assert s.A.shape[1] == 4 and s.C.shape == (4, s.video.T)
    # the other loops need nothing new
    del log[:]
    b.update_temporal_batch(); b.update_background_batch()
    assert [(t, n) for (t, n, _) in log if n in ("update_temporal_parallel", "update_background_parallel")] == \
        [(m, "update_temporal_parallel") for m in range(3)] + [(m, "update_background_parallel") for m in range(3)]
    b.concatenate_temporal_batch()
    assert b.C.shape == b.C_raw.shape == (4, 200) and b.S is None
