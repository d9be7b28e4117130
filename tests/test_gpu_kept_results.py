"""Results that outlive a call (csrc/kept_results.hpp; DESIGN.md, "Lane state and kept results").

A deferred cnmfe_update_spatial leaves its result in four scratch slots of the patch's lane; the record beside them (KeptSpatial) is voided by whatever takes a
slot, so a fetch returns either that result -- np.array_equal to the same update with A_out given -- or CNMFE_ESTATE, never another call's data:

* a temporal, fast-temporal or post-processing call on the lane takes the value slot: the fetch is refused (include/cnmfe.h, cnmfe_update_spatial);
* cnmfe_deconv_temporal takes the pattern slots only: the plain fetch still serves, a projection queued ahead (cnmfe_temporal_early_project) is declined;
* the record is per lane: a temporal update on ANOTHER lane leaves it alone.

Option lanes may change until the first patch exists: the count in force is what cnmfe_get_option("lanes_live") reports, and a run after 2 -> 3 equals lanes = 1.

Shapes: a 24 x 22 field of view, T = 64, K = 4, ring radius 3; the two-lane cases split it into two 24 x 11 patches."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

D1, D2, T, K, R, SEED = 24, 22, 64, 4, 3, 11


class _Ctx:
    """an engine with the video uploaded, the ring fitted and the residual of every patch requested: ready for cnmfe_update_spatial"""

    def __init__(self, lanes=1, pdims=(D1, D2)):
        from cnmf_e_amd import synth
        from cnmf_e_amd.engine import Engine
        from cnmf_e_amd.sources2d import PatchedVideo, Sources2D, Options
        f = synth.make_factors(D1, D2, T, K, SEED, gSig=1.5, gSiz=7, min_sep=4)
        self.eng = Engine(0)
        try:
            if lanes > 1:
                self.eng.set_option("lanes", lanes)
            self.video = PatchedVideo(D1, D2, T, list(pdims), R, self.eng)
            self.video.upload_from_full(synth.make_video(f, np.float32))
            self.s = Sources2D(self.video, Options(ring_radius=R, spatial_algorithm="hals", maxIter=2), f.A_init, f.C_init, f.sn)
            self.s.update_background_parallel()
            self.IND = self.s._search_location_csc(self.s.options.se)
            for idx in self.video.owned:
                self.s._residual(idx, None, None)
        except Exception:
            self.eng.close()
            raise

    def args(self, n):
        """(patch id, A, C, IND) of the n-th patch, on its own pixels and neurons"""
        idx = self.video.owned[n]
        ind, IND_p = self.s._slice(self.IND, idx, "patch")
        assert ind.size > 0, "patch %d holds no neuron" % n
        A_p = self.s._slice(self.s.A, idx, "patch", cols=ind)[1]
        return self.video.pid[idx], A_p, np.ascontiguousarray(np.asarray(self.s.C, dtype=np.float32)[ind]), IND_p

    def spatial(self, n, defer):
        pid, A_p, C_p, IND_p = self.args(n)
        return self.eng.update_spatial(pid, "hals", A_p, C_p, IND_p, None, 3, defer=defer)

    def temporal(self, n):
        pid, A_p, C_p, _ = self.args(n)
        return self.eng.hals_temporal(pid, A_p, C_p, maxIter=2)

    def close(self):
        self.eng.close()


@pytest.fixture(scope="module")
def direct():
    """the reference, computed once: the spatial update of the one-patch field of view and of the first of two patches with A_out given (read-only)"""
    out = {}
    for name, pdims in (("one", (D1, D2)), ("two", (D1, D2 // 2))):
        c = _Ctx(pdims=pdims)
        try:
            A = c.spatial(0, defer=False)
            assert np.all(np.isfinite(A.data)) and np.count_nonzero(A.data) > 0
            A.data.setflags(write=False)
            out[name] = A
        finally:
            c.close()
    return out


def _same(A, B):
    assert np.array_equal(A.indptr, B.indptr) and np.array_equal(A.indices, B.indices) and np.array_equal(A.data, B.data), float(np.abs(A.data - B.data).max())


def _refused(fetch):
    from cnmf_e_amd._lib import CnmfeError
    with pytest.raises(CnmfeError) as e:
        fetch()
    assert "no deferred spatial update" in str(e.value), str(e.value)


def test_deferred_fetch_equals_the_direct_update(direct):
    c = _Ctx()
    try:
        _same(c.spatial(0, defer=True)(), direct["one"])
    finally:
        c.close()


def _take_temporal(c):
    c.temporal(0)


def _take_fast_temporal(c):
    pid, A_p, _, _ = c.args(0)
    c.eng.fast_temporal(pid, A_p)


def _take_post_process(c):
    _, A_p, _, _ = c.args(0)
    assert A_p.nnz > 0                                         # (with nnz = 0 the call returns before it touches the slots)
    c.eng.post_process_spatial(A_p, D1, D2)


@pytest.mark.parametrize("take", [_take_temporal, _take_fast_temporal, _take_post_process], ids=["hals_temporal", "fast_temporal", "post_process_spatial"])
def test_fetch_after_the_value_slot_was_taken_is_refused(take):
    c = _Ctx()
    try:
        fetch = c.spatial(0, defer=True)
        take(c)
        _refused(fetch)
        _refused(lambda: fetch(connected_fov=(D1, D2)))
    finally:
        c.close()


def test_deconv_temporal_takes_the_pattern_only(direct):
    from cnmf_e_amd import _lib as L
    from cnmf_e_amd.engine import _csc, _p
    c = _Ctx()
    try:
        fetch = c.spatial(0, defer=True)
        _, _, C_p, IND_p = c.args(0)
        c.eng.deconv_temporal(C_p, dict(type="ar1", method="foopsi"))
        _same(fetch(), direct["one"])                           # the values stay ...
        _refused(lambda: fetch(connected_fov=(D1, D2)))          # ... the pattern the connectivity kernel reads does not
        Kp, icp, iri, _ = _csc(IND_p.astype(np.float32), D1 * D2)
        before, tk = c.eng.counter("temporal_early_declined"), C.c_int64(-1)
        L.check(L.lib.cnmfe_temporal_early_project(c.eng._ctx, Kp, _p(icp, L.i64p), _p(iri, L.i32p), C.byref(tk)))
        assert tk.value == 0 and c.eng.counter("temporal_early_declined") == before + 1
    finally:
        c.close()


def test_the_record_is_per_lane(direct):
    c = _Ctx(lanes=2, pdims=(D1, D2 // 2))
    try:
        assert len(c.video.owned) == 2 and c.eng.counter("lanes_live") == 2
        fetch = c.spatial(0, defer=True)
        c.temporal(1)                                            # patch 1 runs on lane 1: lane 0's slots are not touched
        _same(fetch(), direct["two"])
    finally:
        c.close()


def test_lanes_change_until_the_first_patch():
    from cnmf_e_amd.engine import Engine
    from test_gpu_lanes import _run, _same as same
    eng = Engine(0)
    try:
        assert eng.counter("lanes_live") == 1
        eng.set_option("lanes", 2); eng.set_option("lanes", 3)
        assert eng.counter("lanes_live") == 3
        eng.set_option("lanes", 3)
        assert eng.counter("lanes_live") == 3
        eng.set_option("lanes", 2); eng.set_option("lanes", 1)
        assert eng.counter("lanes_live") == 1
    finally:
        eng.close()
    case = ((48, 44), [24, 22], 300, 8, 5, 31, dict(spatial_algorithm="hals", maxIter=3))
    ref, rss1 = _run(1, *case)
    got, rss3 = _run(2, *case, opts={"lanes": 3})              # (_run sets lanes = 2, then the options: 2 -> 3 before any patch)
    for it, ((W1, b1, A1, C1, sn1), (W3, b3, A3, C3, sn3)) in enumerate(zip(ref, got)):
        for p, (a, b) in enumerate(zip(W1, W3)):
            same(b, a, "W of patch %d, iteration %d" % (p, it))
        same(b3, b1, "b0_new %d" % it); same(A3, A1, "A %d" % it); same(C3, C1, "C %d" % it); same(sn3, sn1, "sn %d" % it)
    assert rss1 == rss3, (rss1, rss3)
