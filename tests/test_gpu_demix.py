"""orderROIs, demixed_frames and the two kernels behind them (cnmfe.h section (f) and cnmfe_trace_order_stats; csrc/demix.hpp, csrc/merge.hpp) on the engine, against
tests/demix_oracle.py on the fixture of tests/demix_cases.py.

1. the six panels against the oracle holding the ENGINE'S model (A, C, A_prev, C_prev, W, b0, b0_new: the expression is what is compared), bg_ssub 1 and 2,
   frame_range = (6, 203), kt = 3.  Bounds: max error relative to the oracle panel's max |.|, 10 x the value observed on the MI355X rounded up to one digit, never
   above 1e-4; bg never above the 5e-7 of test_gpu_parity.py::test_reconstruct_background_parity.  mixed: equal wherever the float64 value is farther than 0.05 from
   a rounding boundary, within one count elsewhere.
2. checks without a tolerance: bg is reconstruct_background's, signal = raw - bg in fp32, two calls, two lanes, stride 1 against stride 3, the resident C_raw,
   no neurons, a neuron that lies in the halo only
3. after a deconvolving update_temporal_parallel: no K x T upload, the oracle's order, the permuted state, and the next iteration from it
4. cnmfe_trace_order_stats against float64 NumPy
5. refusals

Observed on MI355X, bg_ssub = 1 / 2:
  raw 0.0 / 0.0, bg 1.26e-7 / 8.6e-8, signal 1.09e-5 / 6.7e-6, denoised 5.3e-8 / 5.4e-8, residual 4.34e-5 / 2.03e-5; mixed: none of the 348 480 samples differs
  (98.7 % of them lie farther than 0.05 from a rounding boundary).  cnmfe_trace_order_stats against float64 NumPy: 3.6e-16 relative."""
import numpy as np
import pytest
import scipy.sparse as sp

import demix_cases as dc
import demix_oracle as do

pytestmark = pytest.mark.gpu

CAP = 1e-4
# 10 x observed, one digit up, never above CAP (bg: never above test_reconstruct_background_parity's 5e-7).  raw: the centred video plus its mean gave the fp32
# recording back exactly, so nothing is allowed; signal (10 x 1.09e-5) and residual (10 x 4.34e-5) stop at the cap -- both are differences of two fp32 values near
# 1000 (half an ulp there is 3e-5) measured against the far smaller largest entry of their own panel
BOUNDS = {"raw": 0.0, "bg": 5e-7, "signal": CAP, "denoised": 6e-7, "residual": CAP}
BOUND_STATS = 4e-15                 # 10 x the observed 3.6e-16, one digit up (fp64 sums of 64 .. 1000 terms against NumPy's pairwise ones)
PANELS = ("raw", "bg", "signal", "denoised", "residual")


def _fresh_engine():
    from cnmf_e_amd.engine import Engine
    return Engine(0)


class _State:
    """the recording after one iteration on an engine of its own"""

    def __init__(self, bg_ssub=1, lanes=1, **opts):
        from cnmf_e_amd.sources2d import PatchedVideo, Sources2D, Options
        self.eng = _fresh_engine()
        self.f, self.Y = dc.recording()
        r = dc.radius(bg_ssub)
        if lanes > 1:
            self.eng.set_option("lanes", lanes)
        video = PatchedVideo(dc.D1, dc.D2, dc.T, dc.PATCH, r, self.eng)
        video.upload_from_full(self.Y)
        self.s = Sources2D(video, Options(ring_radius=r, maxIter=3, bg_ssub=bg_ssub, **opts), self.f.A_init, self.f.C_init, self.f.sn)
        self.iterate()

    def iterate(self):
        for step in ("update_background_parallel", "update_spatial_parallel", "update_temporal_parallel"):
            getattr(self.s, step)()

    def close(self):
        self.eng.close()


@pytest.fixture(scope="module")
def plain():
    st = {b: _State(b) for b in (1, 2)}
    yield st
    for x in st.values():
        x.close()


@pytest.fixture(scope="module")
def deconv():
    st = _State(1, deconv_flag=True)
    yield st
    st.close()


def _oracle_with_the_engines_model(st, bg_ssub):
    import cnmfe_oracle as orc
    s = st.s
    o = orc.OracleSources2D(st.Y.T.reshape(dc.D1, dc.D2, dc.T, order="F"), dc.D1, dc.D2, dc.T, dc.PATCH, dc.radius(bg_ssub), st.f.A_init.astype(np.float32),
                            st.f.C_init, st.f.sn, maxIter=3, bg_ssub=bg_ssub)
    o.A, o.C, o.C_raw = sp.csc_matrix(s.A).astype(np.float64), np.asarray(s.C, dtype=np.float64), np.asarray(s.C_raw, dtype=np.float64)
    o.A_prev, o.C_prev = sp.csc_matrix(s.A_prev).astype(np.float64), np.asarray(s.C_prev, dtype=np.float64)
    for idx in s.video.owned:
        o.W[idx] = s.get_W(idx).astype(np.float64); o.b0[idx] = np.asarray(s.get_b0(idx), dtype=np.float64)
    o.b0_new = np.asarray(s.b0_new, dtype=np.float64)
    return o


def _flat(ch, name):
    a = ch[name]
    return a.reshape((dc.D1 * dc.D2,) + a.shape[2:], order="F")


def _all(s, **kw):
    """one chunk holding every displayed frame"""
    chunks = list(s.demixed_frames(chunk=1000, **kw))
    assert len(chunks) == 1
    return chunks[0]


# ---- 1. the panels against the oracle ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bg_ssub", [1, 2])
def test_panels_against_the_oracle(plain, bg_ssub, observed):
    st = plain[bg_ssub]
    s = st.s
    K = s.A.shape[1]
    col = dc.colors(K)
    ch = _all(s, kt=dc.KT, frame_range=dc.FRAME_RANGE, amp_ac=dc.AMP_AC, colors=col)
    assert np.array_equal(ch["frames"], dc.frames() + 1)
    o = _oracle_with_the_engines_model(st, bg_ssub)
    ref = do.panels(o, dc.frames(), o.C, col, dc.AMP_AC)
    errs = {}
    for name in PANELS:
        got = _flat(ch, name)
        assert got.dtype == np.float32 and got.shape == ref[name].shape
        errs[name] = float(np.abs(got - ref[name]).max() / np.abs(ref[name]).max())
    got = _flat(ch, "mixed").astype(np.int64)
    want = ref["mixed"].astype(np.int64)
    far = do.rounding_distance(ref["mixed_double"]) > dc.MIXED_MARGIN
    ndiff = int((got != want).sum())
    print("panels bg_ssub=%d: %s; mixed samples that differ: %d of %d (far from a boundary: %.4f)"
          % (bg_ssub, "  ".join("%s %.3e" % kv for kv in errs.items()), ndiff, got.size, far.mean()))
    observed["demix_panels_ssub%d" % bg_ssub] = dict(errs, mixed_differ=ndiff)
    assert got.shape == want.shape and _flat(ch, "mixed").dtype == np.uint16
    assert far.mean() > 0.98 and want.max() > 0
    assert np.array_equal(got[far], want[far])
    assert np.abs(got - want).max() <= 1
    for name in PANELS:
        assert errs[name] <= BOUNDS[name], (name, errs[name])


# ---- 2. checks without a tolerance --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bg_ssub", [1, 2])
def test_exact_relations(plain, bg_ssub):
    s = plain[bg_ssub].s
    K = s.A.shape[1]
    kw = dict(frame_range=dc.FRAME_RANGE, amp_ac=dc.AMP_AC, colors=dc.colors(K))
    a = _all(s, kt=dc.KT, **kw)
    Ybg = s.reconstruct_background(dc.FRAME_RANGE)
    assert np.array_equal(a["bg"], Ybg[:, :, ::dc.KT])                       # the bits of reconstruct_background
    assert np.array_equal(a["signal"], a["raw"] - a["bg"])                   # one fp32 subtraction
    Y = plain[bg_ssub].Y.T.reshape(dc.D1, dc.D2, dc.T, order="F")[:, :, dc.frames()]
    assert np.abs(a["raw"] - Y).max() <= 2.0 ** -22 * np.abs(Y).max()        # Yc + Ymean: two fp32 roundings of the video
    b = _all(s, kt=dc.KT, **kw)
    one = _all(s, kt=1, **kw)
    parts = list(s.demixed_frames(kt=dc.KT, chunk=7, **kw))                  # chunks that start anywhere in a quad
    for name in PANELS + ("mixed",):
        assert np.array_equal(a[name], b[name]), name                        # two calls
        assert np.array_equal(a[name], one[name][:, :, ::dc.KT]), name       # stride 1 at the frames of stride 3
        assert np.array_equal(a[name], np.concatenate([c[name] for c in parts], axis=2)), name


def test_two_lanes_give_the_bits_of_one(plain):
    st2 = _State(2, lanes=2)
    try:
        K = st2.s.A.shape[1]
        kw = dict(kt=dc.KT, frame_range=dc.FRAME_RANGE, amp_ac=dc.AMP_AC, colors=dc.colors(K))
        a, b = _all(plain[2].s, **kw), _all(st2.s, **kw)
        for name in PANELS + ("mixed",):
            assert np.array_equal(a[name], b[name]), name
    finally:
        st2.close()


def test_no_neurons_and_a_halo_only_neuron(plain):
    """the entry point itself on patch (0, 0): Ksel = 0 gives zero denoised and mixed; a neuron with pixels in the halo only (an empty column of A) changes nothing"""
    st = plain[1]
    s, eng, v = st.s, st.eng, st.s.video
    idx = v.order[0]
    pid, pp = v.pid[idx], v.patch_pix[idx]
    b0_ = s.reconstruct_b0().reshape(-1, order="F")
    b0n = np.asarray(s.b0_new, dtype=np.float64).reshape(-1, order="F")
    s._background_resident(idx, b0_)
    args = (b0_[v.block_pix[idx]], b0n[pp])
    fr = (5, dc.KT, dc.frames().size)
    ind, A_pp = s._slice(s.A, idx, "patch")
    assert ind.size >= 1
    CC = np.ascontiguousarray(np.asarray(s.C), dtype=np.float32)
    col = dc.colors(CC.shape[0])
    full = eng.demix_frames(pid, *args, A_pp, CC, ind, col[ind], 1000.0, *fr)
    none = eng.demix_frames(pid, *args, None, CC, np.zeros(0, np.int32), np.zeros((0, 3), np.float32), 1000.0, *fr)
    assert not none["denoised"].any() and not none["mixed"].any()
    for name in ("raw", "bg", "signal"):
        assert np.array_equal(none[name], full[name])
    assert np.array_equal(none["residual"], none["signal"])                  # (float)((double)raw - (double)bg - 0) is the fp32 difference: it is exact in fp64
    assert full["denoised"].any() and full["mixed"].any()
    a_h, c_h = dc.halo_neuron()
    assert a_h[v.block_pix[idx]].nnz and not a_h[pp].nnz
    A2 = sp.hstack([A_pp, a_h[pp]], format="csc")
    CC2 = np.concatenate([CC, c_h[None, :]])
    col2 = np.concatenate([col[ind], np.ones((1, 3), np.float32)])
    halo = eng.demix_frames(pid, *args, A2, CC2, np.append(ind, CC.shape[0]), col2, 1000.0, *fr)
    for name in PANELS + ("mixed",):
        assert np.array_equal(halo[name], full[name]), name
    # the bound matrix read where it lies gives what its host copy gives
    bound = eng.demix_frames(pid, *args, A_pp, s.C, ind, col[ind], 1000.0, *fr)
    for name in PANELS + ("mixed",):
        assert np.array_equal(bound[name], full[name]), name
    zero = eng.demix_frames(pid, *args, A_pp, CC, ind, col[ind], 1000.0, 5, dc.KT, 0)
    assert zero["raw"].shape == (0, pp.size) and zero["mixed"].shape == (3, 0, pp.size)


# ---- 3. after a deconvolving temporal update ------------------------------------------------------------------------------------------------
def test_no_upload_and_the_resident_c_raw(deconv):
    s, eng = deconv.s, deconv.eng
    K = s.A.shape[1]
    before = (eng.counter("merge_trace_uploads"), eng.counter("trace_matrix_uploads"))
    kw = dict(kt=dc.KT, frame_range=dc.FRAME_RANGE, colors=dc.colors(K))
    raw = _all(s, use_craw=True, **kw)                                       # amp_ac by default: max(CC) from the engine's statistics
    den = _all(s, **kw)
    assert (eng.counter("merge_trace_uploads"), eng.counter("trace_matrix_uploads")) == before
    assert eng.residents_are(s.C, s.C_raw, s.S)
    A = sp.csr_matrix(s.A).astype(np.float64)
    for ch, CC in ((raw, s.C_raw), (den, s.C)):
        want = np.asarray(A @ np.asarray(CC, dtype=np.float64)[:, dc.frames()]).astype(np.float32)
        assert np.abs(_flat(ch, "denoised") - want).max() <= 2.0 ** -22 * np.abs(want).max()
    assert not np.array_equal(raw["denoised"], den["denoised"])
    host = _all(s, use_craw=True, amp_ac=do.default_amp_ac(s.A, np.asarray(s.C_raw)), **kw)
    assert np.abs(host["mixed"].astype(np.int64) - raw["mixed"].astype(np.int64)).max() <= 1      # (the default amp_ac agrees to the last bits of a double)


def test_order_rois_after_a_deconvolving_update():
    a, b = _State(1, deconv_flag=True), _State(1, deconv_flag=True)
    try:
        s, eng = a.s, a.eng
        K = s.A.shape[1]
        s.ids, s.tags = np.arange(10, 10 + K), np.arange(K, dtype=np.uint16)
        old = dict(A=sp.csc_matrix(s.A).toarray(), C=np.array(s.C), C_raw=np.array(s.C_raw), S=np.array(s.S), kp=np.array(s.P["kernel_pars"]), ids=s.ids, tags=s.tags)
        for k in ("A", "C", "C_raw", "S"):
            assert np.array_equal(old[k], sp.csc_matrix(getattr(b.s, k)).toarray() if k == "A" else np.asarray(getattr(b.s, k))), k      # two engines, one trajectory
        A_prev, C_prev = s.A_prev, s.C_prev
        before = (eng.counter("merge_trace_uploads"), eng.counter("trace_matrix_uploads"))
        for name in ("pnr", "snr"):
            cur = dict(A=sp.csc_matrix(s.A).toarray(), C=np.array(s.C), C_raw=np.array(s.C_raw), S=np.array(s.S), kp=np.array(s.P["kernel_pars"]), ids=s.ids, tags=s.tags)
            want, val = do.order_rois(name, cur["A"], cur["C"], cur["C_raw"])
            # (a trace the deconvolution found no spike in has C = C_raw on the engine: its criterion is Inf and sorts first; one such value cannot tie)
            assert do.margin(val) > dc.ORDER_MARGIN and not np.isnan(val).any() and np.isinf(val).sum() <= 1
            srt = s.orderROIs(name)
            assert np.array_equal(srt, want), name
            assert np.array_equal(sp.csc_matrix(s.A).toarray(), cur["A"][:, srt])
            for k, now in (("C", s.C), ("C_raw", s.C_raw), ("S", s.S), ("kp", s.P["kernel_pars"]), ("ids", s.ids), ("tags", s.tags)):
                assert np.array_equal(np.asarray(now), cur[k][srt]), (name, k)
        assert (eng.counter("merge_trace_uploads"), eng.counter("trace_matrix_uploads")) == before
        assert s.A_prev is A_prev and s.C_prev is C_prev
        total = np.array([np.flatnonzero((old["C"] == row).all(axis=1))[0] for row in np.asarray(s.C)])      # the composition of the two orders
        # the same state from the host: set_components of the permuted matrices on the second engine
        t = b.s
        t.set_components(sp.csc_matrix(old["A"][:, total]), old["C"][total], old["C_raw"][total])
        t.S = old["S"][total]; t.P["kernel_pars"] = old["kp"][total]
        if t.P.get("neuron_sn") is not None:
            t.P["neuron_sn"] = np.asarray(t.P["neuron_sn"])[total]
        a.iterate(); b.iterate()
        for k in ("A", "C", "C_raw", "S"):
            x, y = getattr(s, k), getattr(t, k)
            assert np.array_equal(sp.csc_matrix(x).toarray() if k == "A" else np.asarray(x), sp.csc_matrix(y).toarray() if k == "A" else np.asarray(y)), k
        assert np.array_equal(np.asarray(s.P["kernel_pars"]), np.asarray(t.P["kernel_pars"]))
    finally:
        a.close(); b.close()


def test_order_rois_tie_and_nan(plain):
    s = plain[1].s
    C, R = dc.tie_nan_traces()
    A, Cm, Cr = s.A, s.C, s.C_raw
    try:
        s.set_components(A, C, R)
        want, val = do.order_rois("snr", A, C, R)
        assert np.isnan(val[2]) and val[1] == val[4]
        assert np.array_equal(s.orderROIs("snr"), want)
        inv = np.argsort(want)
        assert np.array_equal(s.orderROIs(inv), inv) and np.array_equal(np.asarray(s.C), C)      # an explicit permutation: back to the first order
        with pytest.raises(ValueError):
            s.orderROIs([0, 0, 1, 2, 3, 4])
    finally:
        s.set_components(A, Cm, Cr)


# ---- 4. the statistics ------------------------------------------------------------------------------------------------------------------
def test_trace_order_stats_against_numpy(deconv, observed):
    eng = _fresh_engine()
    try:
        rng = np.random.default_rng(7)
        worst = 0.0
        for K, T in ((5, 203), (3, 1000), (2, 64)):                          # T % 4 = 3; more than one pass of the 256 threads; one short trace
            C = (rng.random((K, T)) * 30 + 100).astype(np.float32)           # a large mean: the two-pass variance matters
            R = (C + rng.standard_normal((K, T)).astype(np.float32)).astype(np.float32)
            eng.traces_load(C, R)
            got = eng.trace_order_stats()
            ref = do.order_stats(C, R)
            assert got.shape == (K, 7)
            assert np.array_equal(got[:, [3, 6]], ref[:, [3, 6]])            # the maxima are exact
            assert np.all(ref != 0)
            worst = max(worst, float((np.abs(got - ref) / np.abs(ref)).max()))
            assert np.array_equal(eng.trace_order_stats(), got)              # two calls
        print("trace_order_stats: max relative error %.3e" % worst)
        observed["trace_order_stats"] = worst
        assert worst <= BOUND_STATS, worst
        Ct, Rt = dc.tie_nan_traces()
        eng.traces_load(Ct, Rt)
        q = eng.trace_order_stats()
        assert q[2, 1] == 0 and q[2, 2] == 0 and q[5, 2] == 0 and np.array_equal(q[1], q[4])      # a constant row has no variance at all; identical rows, identical bits
    finally:
        eng.close()
    q = deconv.eng.trace_order_stats()                                        # ... and on the residents a deconvolving update leaves
    ref = do.order_stats(np.asarray(deconv.s.C), np.asarray(deconv.s.C_raw))
    assert np.all(np.abs(q - ref) <= BOUND_STATS * np.abs(ref))               # (a trace without a spike has C_raw = C: var(C_raw - C) is 0 on both sides)


# ---- 5. refusals --------------------------------------------------------------------------------------------------------------------------
def test_refusals(plain):
    from cnmf_e_amd._lib import CnmfeError
    from cnmf_e_amd.sources2d import PatchedVideo
    st = plain[1]
    s, eng, v = st.s, st.eng, st.s.video
    idx = v.order[0]
    pid, pp = v.pid[idx], v.patch_pix[idx]
    b0_ = s.reconstruct_b0().reshape(-1, order="F")
    b0n = np.asarray(s.b0_new, dtype=np.float64).reshape(-1, order="F")
    s._background_resident(idx, b0_)
    args = (b0_[v.block_pix[idx]], b0n[pp])
    ind, A_pp = s._slice(s.A, idx, "patch")
    CC = np.ascontiguousarray(np.asarray(s.C), dtype=np.float32)
    col = dc.colors(CC.shape[0])[ind]

    def refused(code, *frames, A=A_pp, rows=ind, engine=eng, p=pid):
        with pytest.raises(CnmfeError, match="error %d" % code):
            engine.demix_frames(p, *args, A, CC, rows, col, 1000.0, *frames)
    ok = eng.demix_frames(pid, *args, A_pp, CC, ind, col, 1000.0, dc.T - 1, 1, 1)      # frame T itself is served
    refused(-1, dc.T, 1, 1)                                                  # a frame >= T
    refused(-1, dc.T - 4, 3, 3)                                              # ... reached by the stride
    refused(-1, 0, 0, 4)                                                     # stride = 0
    refused(-1, 0, 1, -1)                                                    # nframes < 0
    refused(-1, -1, 1, 2)
    assert s.C is eng._bound                                                 # the bound matrix with a row beyond it
    with pytest.raises(CnmfeError, match="error -1"):
        eng.demix_frames(pid, *args, A_pp, s.C, np.full(ind.size, CC.shape[0]), col, 1000.0, 0, 1, 2)
    e2 = _fresh_engine()                                                     # no residual of the block's neurons
    try:
        v2 = PatchedVideo(dc.D1, dc.D2, dc.T, dc.PATCH, dc.radius(1), e2)
        v2.upload_from_full(st.Y)
        for i2 in v2.owned:
            e2.ring_init(v2.pid[i2], dc.radius(1))
        refused(-4, 0, 1, 2, engine=e2, p=v2.pid[idx])
        with pytest.raises(CnmfeError, match="error -4"):
            _stats_without_residents(e2)                                     # no C, C_raw in the context
    finally:
        e2.close()
    again = eng.demix_frames(pid, *args, A_pp, CC, ind, col, 1000.0, dc.T - 1, 1, 1)   # the context still works, and gives what it gave
    for name in PANELS + ("mixed",):
        assert np.array_equal(ok[name], again[name])
    with pytest.raises(ValueError):
        s.orderROIs(np.arange(s.A.shape[1]) + 1)                             # not a permutation of 0 .. K - 1
    with pytest.raises(NotImplementedError):
        s.orderROIs("circularity")


def _stats_without_residents(e):
    import ctypes as C
    from cnmf_e_amd import _lib as L
    out = np.zeros(21)
    L.check(L.lib.cnmfe_trace_order_stats(e._ctx, 3, out.ctypes.data_as(L.f64p)))
