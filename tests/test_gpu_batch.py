"""Batch mode on the device (cnmf_e_amd/batch.py, cnmfe_trace_energy, cnmfe_traces_grow) on the fixtures of tests/batch_cases.py: 32 x 32 pixels, ring radius 4,
one recording cut into batches of 96, 128 and 80 frames; once one patch, once 2 x 2 patches, once with deconv_flag.

1. the batch methods (all but update_spatial_batch) against the same sequence written out with the single-recording methods on a second set of engines: bit-equal --
   the methods only order calls that are each deterministic; where C grows the hand sequence pads on the host.
2. update_spatial_batch against the float64 restatement (batch_cases.weighted_average) of the batches' own updates: within one float32 ulp of the restatement rounded to
   float32; the last batch keeps its own update unless spread_all; a neuron silenced in every batch is an empty column and is named.
3. cnmfe_trace_energy: relative error <= 2 T 2^-53 (the plain summation bound; the tree order only improves on it), equal bits on every call and under lanes = 2.
4. cnmfe_traces_grow: old rows keep their bits, new rows are zero, no upload, the next temporal update equals the one from the host-padded C on an engine that never
   grew; the error codes.
5. K grows across batches by the search itself (batch_cases.GROW, whose condition tests/test_batch_host.py::test_grow_fixture checks on the CPU): a neuron silent in
   batch 1 is found by batch 2's second pass; then every batch has the same K, ids continue from P.k_ids, the footprint correlates above 0.8 with the truth and the
   neuron's batch-1 trace stays below 3 neuron_sn.
6. the demo's sequence (demo_batch_1p.m:123-142) end to end with three contexts alive, closed in another order than they were made."""
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

pytestmark = pytest.mark.gpu

CONFIGS = {"one_patch": dict(case="late", pdims=[32, 32], deconv=False), "2x2": dict(case="late", pdims=[16, 16], deconv=False),
           "deconv": dict(case="plain", pdims=[32, 32], deconv=True)}


def _make_batches(cfg, lanes=1):
    """one fresh (engine, video, Sources2D) per batch: A = d x 0, sn from its own estimate_noise (what Sources2DBatch.from_full makes, with this file's cuts)"""
    from cnmf_e_amd.engine import Engine
    from cnmf_e_amd.sources2d import PatchedVideo, Sources2D
    f, Y = bc.make(cfg["case"])
    opts = bc.options(deconv=cfg["deconv"])
    d = bc.D1 * bc.D2
    out = []
    try:
        for t0, t1 in bc.ranges():
            eng = Engine(0)
            out.append(eng)
            if lanes > 1:
                eng.set_option("lanes", lanes)
            video = PatchedVideo(bc.D1, bc.D2, t1 - t0, cfg["pdims"], bc.RADIUS, eng)
            video.upload_from_full(Y[t0:t1])
            s = Sources2D(video, opts, sp.csc_matrix((d, 0), dtype=np.float32), np.zeros((0, t1 - t0), np.float32), np.zeros(d, np.float32))
            s.estimate_noise()
            out[-1] = s
    except Exception:
        for x in out:
            (x.engine if hasattr(x, "engine") else x).close()
        raise
    return out, opts


def _close(batches):
    for s in batches:
        s.engine.close()


def _state(s):
    """everything test 1 compares of one batch, as plain arrays"""
    S = getattr(s, "S", None)
    A = sp.csc_matrix(s.A)
    A.sort_indices()
    return dict(A=(A.shape, A.indptr.copy(), A.indices.copy(), A.data.copy()), C=np.array(s.C, dtype=np.float32), C_raw=np.array(s.C_raw, dtype=np.float32),
                S=None if S is None else np.array(S, dtype=np.float32), ids=np.array(s.ids), tags=np.array(s.tags),
                W={idx: s.get_W(idx) for idx in s.video.owned}, b0={idx: s.get_b0(idx).copy() for idx in s.video.owned})


def _same_bits(x, y):
    return x.shape == y.shape and x.dtype == y.dtype and np.array_equal(np.ascontiguousarray(x).view(np.uint8), np.ascontiguousarray(y).view(np.uint8))


def _assert_same_state(a, b, what):
    for i, (u, v) in enumerate(zip(a["A"][1:], b["A"][1:])):
        assert a["A"][0] == b["A"][0] and _same_bits(u, v), (what, "A", i)
    for n in ("C", "C_raw", "S"):
        assert (a[n] is None) == (b[n] is None) and (a[n] is None or _same_bits(a[n], b[n])), (what, n)
    assert np.array_equal(a["ids"], b["ids"]) and np.array_equal(a["tags"], b["tags"]), (what, "ids / tags")
    for idx in a["W"]:
        Wa, Wb = a["W"][idx], b["W"][idx]
        assert np.array_equal(Wa.indptr, Wb.indptr) and np.array_equal(Wa.indices, Wb.indices) and _same_bits(Wa.data, Wb.data), (what, "W", idx)
        assert _same_bits(a["b0"][idx], b["b0"][idx]), (what, "b0", idx)


def _pad(X, K):
    X = np.asarray(X, dtype=np.float32)
    return np.concatenate([X, np.zeros((K - X.shape[0], X.shape[1]), np.float32)])


def _hand_grow(s, A, ids, tags, k_ids):
    """the second loop of initComponents_batch.m:97-106 / update_temporal_batch.m:24-27 with what Sources2D had before batch mode: padded on the host, bound again"""
    K = A.shape[1]
    S = getattr(s, "S", None)
    if S is not None and np.shape(S)[0] == s.C.shape[0]:
        s.S = _pad(S, K)
    for n in ("kernel_pars", "neuron_sn"):
        if s.P.get(n) is not None and len(s.P[n]) == s.C.shape[0]:
            v = np.asarray(s.P[n]).ravel()
            s.P[n] = np.concatenate([v, np.zeros(K - v.size, v.dtype)])
    s.set_components(A, _pad(s.C, K), None if s.C_raw is s.C else _pad(s.C_raw, K))
    s.ids, s.tags, s.P["k_ids"] = np.array(ids), np.array(tags), int(k_ids)


def _hand_init(batches):
    """initComponents_batch.m:36-113 written out"""
    A = ids = tags = k_ids = None
    for m, s in enumerate(batches):
        if m == 0:
            s.initComponents_parallel(None)
        else:
            s.A = A; s.ids = np.array(ids); s.tags = np.array(tags); s.P["k_ids"] = int(k_ids)
            if A.shape[1]:
                s.initTemporal()
        s.update_background_parallel()
        s.initComponents_residual_parallel()
        A, ids, tags, k_ids = s.A, s.ids, s.tags, s.P["k_ids"]
    for s in batches:
        if s.A.shape[1] == A.shape[1]:
            continue
        _hand_grow(s, A, ids, tags, k_ids)
        s.update_temporal_parallel()
    return A, ids, tags, k_ids


def _extra_column(A, f):
    """A with one more footprint: the synthetic start of the last true neuron, which no batch's A holds in this form"""
    a = sp.csc_matrix(f.A_init.tocsc()[:, [f.K - 1]], dtype=np.float32)
    out = sp.hstack([sp.csc_matrix(A), a], format="csc", dtype=np.float32)
    out.sort_indices()
    return out


@pytest.mark.parametrize("name", list(CONFIGS))
def test_batch_methods_equal_the_hand_sequence(name):
    from cnmf_e_amd.batch import Sources2DBatch
    cfg = CONFIGS[name]
    f, _ = bc.make(cfg["case"])
    bat, opts = _make_batches(cfg)
    hand, _o2 = _make_batches(cfg)
    try:
        b = Sources2DBatch(bat, opts)
        ups = [s.engine.counter("trace_matrix_uploads") for s in bat]
        b.initComponents_batch()
        A, ids, tags, k_ids = _hand_init(hand)
        Ks = [s.A.shape[1] for s in bat]
        print("%s: K per batch after initComponents_batch %s, parent %d, ids %s" % (name, Ks, b.A.shape[1], b.ids.tolist()))
        assert b.A.shape[1] > 0 and Ks == [b.A.shape[1]] * 3 and b.P["k_ids"] == k_ids == len(b.ids) and np.array_equal(b.ids, np.arange(1, len(b.ids) + 1))
        assert all(s.C.shape == (b.A.shape[1], s.video.T) for s in bat)
        for m in range(3):
            _assert_same_state(_state(bat[m]), _state(hand[m]), (name, "init", m))
            assert np.array_equal(bat[m].ids, b.ids) and np.array_equal(bat[m].tags, b.tags)
        # K grows by one footprint everywhere: update_temporal_batch pads on the device, the hand sequence on the host
        A2 = _extra_column(b.A, f)
        b.A = A2
        b.ids = np.concatenate([b.ids, [b.P["k_ids"] + 1]]); b.tags = np.concatenate([b.tags, np.zeros(1, np.uint16)]); b.P["k_ids"] += 1
        ups = [s.engine.counter("trace_matrix_uploads") for s in bat]
        for s in bat:
            b._hand_down(s)
        for s in bat:
            K0 = s.C.shape[0]
            s._grow_K(A2.shape[1])
            assert s.C.shape[0] == K0 + 1 and s.engine._bound is s.C
        assert [s.engine.counter("trace_matrix_uploads") for s in bat] == ups               # handing A down and growing C moved no K x T matrix
        b.update_temporal_batch()
        for s in hand:
            _hand_grow(s, A2, b.ids, b.tags, b.P["k_ids"])
            s.update_temporal_parallel()
        for m in range(3):
            _assert_same_state(_state(bat[m]), _state(hand[m]), (name, "temporal", m))
        b.update_background_batch()
        for s in hand:
            s.update_background_parallel()
        pairs = b.correlation_pnr_batch()
        for m in range(3):
            _assert_same_state(_state(bat[m]), _state(hand[m]), (name, "background", m))
            Cn, PNR = hand[m].correlation_pnr_parallel()
            assert _same_bits(pairs[m][0], Cn) and _same_bits(pairs[m][1], PNR) and bat[m].Cn is pairs[m][0] and bat[m].PNR is pairs[m][1]
        b.concatenate_temporal_batch()
        K = b.A.shape[1]
        assert b.C.shape == b.C_raw.shape == (K, bc.T) and b.C.dtype == b.C_raw.dtype == np.float32 and (b.S is not None) == cfg["deconv"]
        for m, (t0, t1) in enumerate(bc.ranges()):
            st = _state(hand[m])
            assert _same_bits(np.ascontiguousarray(b.C[:, t0:t1]), st["C"]) and _same_bits(np.ascontiguousarray(b.C_raw[:, t0:t1]), st["C_raw"])
            if cfg["deconv"]:
                assert _same_bits(np.ascontiguousarray(b.S[:, t0:t1]), st["S"])
    finally:
        _close(bat); _close(hand)


def test_update_spatial_batch():
    from cnmf_e_amd.batch import Sources2DBatch
    cfg = CONFIGS["2x2"]
    bat, opts = _make_batches(cfg)
    try:
        b = Sources2DBatch(bat, opts)
        b.initComponents_batch()
        K = b.A.shape[1]
        assert K >= 2
        snaps = []

        def snap(s):
            orig = s.update_spatial_parallel

            def wrapped(*a, **k):
                orig(*a, **k)
                snaps.append((sp.csc_matrix(s.A).copy(), np.array(s.C, dtype=np.float32)))
            s.update_spatial_parallel = wrapped
        for s in bat:
            snap(s)
        ups = [s.engine.counter("trace_matrix_uploads") for s in bat]
        dead = b.update_spatial_batch()
        assert [s.engine.counter("trace_matrix_uploads") for s in bat] == ups               # the weights are taken where C lies; a new A re-uploads no C
        want, dead_want = bc.weighted_average([a for a, _ in snaps], [c for _, c in snaps])
        assert dead.size == 0 and dead_want.size == 0
        got = b.A.toarray()
        assert b.A.dtype == np.float32 and bc.within_one_ulp(got, want)
        assert np.array_equal(bat[0].A.toarray(), got) and np.array_equal(bat[1].A.toarray(), got)
        assert np.array_equal(bat[2].A.toarray(), snaps[2][0].toarray()) and not np.array_equal(bat[2].A.toarray(), got)      # the last batch keeps its own (:37)
        assert all(s.engine._bound is s.C for s in bat)
        # the batches go on from the new A: a temporal and a background update run
        b.update_temporal_batch(); b.update_background_batch()
        # spread_all, and a neuron silenced in every batch
        kill = 1
        for s in bat:
            Cz = np.array(s.C, dtype=np.float32); Cz[kill] = 0.0
            s.set_components(s.A, Cz)
        del snaps[:]
        dead = b.update_spatial_batch(spread_all=True)
        want, dead_want = bc.weighted_average([a for a, _ in snaps], [c for _, c in snaps])
        got = b.A.toarray()
        assert dead.tolist() == dead_want.tolist() == [kill]
        assert b.A.indptr[kill + 1] == b.A.indptr[kill] and np.isfinite(got).all() and bc.within_one_ulp(got, want)
        assert all(np.array_equal(s.A.toarray(), got) for s in bat)
    finally:
        _close(bat)


# ---- 3. cnmfe_trace_energy -----------------------------------------------------------------------------------------------------------------------------------
def _energy_ok(e, X):
    ref = (np.asarray(X).astype(np.float64) ** 2).sum(axis=1)
    T = X.shape[1]
    err = np.abs(e - ref)
    assert e.dtype == np.float64 and np.all(err <= T * 2.0 ** -53 * 2 * ref), (X.shape, float((err / np.maximum(ref, 1e-300)).max()))


def _trace_matrix(K, T, seed):
    rng = np.random.default_rng(seed)
    X = (rng.standard_normal((K, T)) * rng.uniform(0.1, 30.0, (K, 1))).astype(np.float32)
    if K > 1:
        X[1] = 0.0                                                            # a silent trace: exactly 0
    return X


def test_trace_energy_host_and_bound():
    from cnmf_e_amd.engine import Engine
    e1, e2 = Engine(0), Engine(0)
    try:
        e2.set_option("lanes", 2)
        assert e2.counter("lanes_live") == 2
        for K in (1, 3, 70):
            for T in (1, 80, 4099):
                X = _trace_matrix(K, T, 100 * K + T)
                a = e1.trace_energy(X)
                _energy_ok(a, X)
                assert _same_bits(e1.trace_energy(X), a) and _same_bits(e2.trace_energy(X), a)      # every call, any lane count
                up = e1.counter("trace_matrix_uploads")
                e1.bind_traces(X); e2.bind_traces(X)
                up_b = e1.counter("trace_matrix_uploads")
                assert up_b == up + 1
                assert _same_bits(e1.trace_energy(X), a) and _same_bits(e2.trace_energy(X), a)      # the bound matrix, read where it lies
                assert e1.counter("trace_matrix_uploads") == up_b
        assert e1.trace_energy(np.zeros((0, 10), np.float32)).shape == (0,)
    finally:
        e1.close(); e2.close()


def _deconv_run(grow_to=None):
    """a small recording after background, spatial and a DECONVOLVING temporal update: C is bound, C_raw and S are the context's residents"""
    from cnmf_e_amd import synth
    from cnmf_e_amd.engine import Engine
    from cnmf_e_amd.sources2d import PatchedVideo, Sources2D, Options
    d1, d2, T, K, r = 32, 32, 203, 5, 4
    f = synth.make_factors(d1, d2, T, K + 3, 3, gSig=1.5, gSiz=7, min_sep=5)
    Y = synth.make_video(f, np.float32)
    eng = Engine(0)
    try:
        video = PatchedVideo(d1, d2, T, [16, 16], r, eng)
        video.upload_from_full(Y)
        s = Sources2D(video, Options(ring_radius=r, maxIter=3, deconv_flag=True), f.A_init.tocsc()[:, :K], f.C_init[:K], f.sn)
        s.update_background_parallel(); s.update_spatial_parallel(); s.update_temporal_parallel()
    except Exception:
        eng.close()
        raise
    A_more = sp.hstack([sp.csc_matrix(s.A), sp.csc_matrix(f.A_init.tocsc()[:, K:], dtype=np.float32)], format="csc", dtype=np.float32)
    A_more.sort_indices()
    return eng, s, A_more


def test_trace_energy_residents():
    eng, s, _ = _deconv_run()
    try:
        assert eng.residents_are(s.C, s.C_raw, s.S)
        up, mu = eng.counter("trace_matrix_uploads"), eng.counter("merge_trace_uploads")
        got = [eng.trace_energy(X) for X in (s.C, s.C_raw, s.S)]
        assert eng.counter("trace_matrix_uploads") == up and eng.counter("merge_trace_uploads") == mu
        for e, X in zip(got, (s.C, s.C_raw, s.S)):
            _energy_ok(e, np.asarray(X, dtype=np.float32))
            assert _same_bits(eng.trace_energy(X), e)
        assert _same_bits(s._trace_energy(), got[0])
    finally:
        eng.close()


# ---- 4. cnmfe_traces_grow ------------------------------------------------------------------------------------------------------------------------------------
def test_traces_grow_keeps_rows_and_uploads_nothing():
    eng, s, A_more = _deconv_run()
    try:
        K, T = s.C.shape
        old = [np.array(X, dtype=np.float32) for X in (s.C, s.C_raw, s.S)]
        kp_old, sn_old = np.array(s.P["kernel_pars"], dtype=np.float32).ravel(), np.array(s.P["neuron_sn"], dtype=np.float32).ravel()
        up = eng.counter("trace_matrix_uploads")
        s._set_A(A_more)
        s._grow_K(K + 3)
        assert eng.counter("trace_matrix_uploads") == up and eng.counter("bound_K") == K + 3
        assert eng._bound is s.C and eng.residents_are(s.C, s.C_raw, s.S)
        for X, o in zip((s.C, s.C_raw, s.S), old):                             # the host objects that stand for the grown matrices
            assert X.shape == (K + 3, T) and _same_bits(np.asarray(X)[:K].copy(), o) and not np.asarray(X)[K:].any()
        assert len(s.P["kernel_pars"]) == len(s.P["neuron_sn"]) == K + 3 and not np.asarray(s.P["kernel_pars"])[K:].any()
        # ... and what the device holds: the energies of the grown matrices, and the matrices themselves through a delete of nothing
        for X, o in zip((s.C, s.C_raw, s.S), old):
            e = eng.trace_energy(X)
            assert _same_bits(e[:K].copy(), eng.trace_energy(o)) and not e[K:].any()
        assert eng.counter("trace_matrix_uploads") == up + 3                   # (the three host matrices just compared against)
        Cn, Rn, Sn, kp, sn = eng.merge_apply([], [], np.arange(K + 3), None)
        for X, o in zip((Cn, Rn, Sn), old):
            assert X.shape == (K + 3, T) and _same_bits(X[:K].copy(), o) and not X[K:].any()
        assert _same_bits(kp[:K].copy(), kp_old) and _same_bits(sn[:K].copy(), sn_old) and not kp[K:].any() and not sn[K:].any()
    finally:
        eng.close()


def test_traces_grow_next_temporal_update():
    eng, s, A_more = _deconv_run()
    eng2, s2, _ = _deconv_run()
    try:
        K = s.C.shape[0]
        s._set_A(A_more); s._grow_K(K + 3)
        s.update_temporal_parallel()
        s2.S = _pad(s2.S, K + 3)                                               # an engine that never grew: the host-padded C
        s2.set_components(A_more, _pad(s2.C, K + 3), _pad(s2.C_raw, K + 3))
        s2.update_temporal_parallel()
        for n in ("C", "C_raw", "S"):
            assert _same_bits(np.array(getattr(s, n), dtype=np.float32), np.array(getattr(s2, n), dtype=np.float32)), n
        assert np.asarray(s.C).shape[0] == K + 3
    finally:
        eng.close(); eng2.close()


def test_traces_grow_error_codes():
    from cnmf_e_amd import _lib as L
    from cnmf_e_amd.engine import Engine
    EINVAL, ESTATE = -1, -4
    eng = Engine(0)
    try:
        assert L.lib.cnmfe_traces_grow(eng._ctx, 4) == ESTATE                  # nothing bound
        X = _trace_matrix(3, 81, 1)
        eng.bind_traces(X)
        assert L.lib.cnmfe_traces_grow(eng._ctx, 2) == EINVAL
        assert L.lib.cnmfe_traces_grow(eng._ctx, 3) == 0 and eng.counter("bound_K") == 3
        C2, R2, S2 = eng.traces_grow(3)
        assert C2 is X and R2 is None and S2 is None
        C5, R5, S5 = eng.traces_grow(5)                                        # no residents: the bound matrix alone
        assert eng._bound is C5 and R5 is None and S5 is None and eng.counter("bound_K") == 5
        e = eng.trace_energy(C5)
        assert _same_bits(e[:3].copy(), eng.trace_energy(X)) and not e[3:].any()
        assert np.array_equal(np.asarray(C5)[:3], X) and not np.asarray(C5)[3:].any()
        # a matrix bound in MATLAB's layout (column-major) grows as well: the device keeps rows either way
        Xc = np.ascontiguousarray(X.T)                                         # T x K C-order == K x T column-major
        L.check(L.lib.cnmfe_traces_bind(eng._ctx, 3, 81, Xc.ctypes.data_as(L.f32p), L.COLMAJOR))
        assert L.lib.cnmfe_traces_grow(eng._ctx, 4) == 0 and eng.counter("bound_K") == 4
        out = np.zeros(4, np.float64)
        L.check(L.lib.cnmfe_trace_energy(eng._ctx, 4, 81, None, L.BOUND, out.ctypes.data_as(L.f64p)))
        assert _same_bits(out[:3].copy(), eng.trace_energy(X)) and out[3] == 0
    finally:
        eng.close()


# ---- 5. K grows across batches -------------------------------------------------------------------------------------------------------------------------------
def test_K_grows_across_batches():
    """Observed on the MI355X: K around the three second passes (5, 5), (5, 6), (6, 7); the late neuron found at (8, 31) (truth (7, 31)); footprint correlation 0.966;
    batch 1 max |C| = 0.0850529 against 3 x neuron_sn = 0.0850956 (a trace without spikes is C_raw - b, deconvTemporal.m:53-55: noise, whose maximum over 96 frames is
    about three sigma by nature)."""
    from cnmf_e_amd.batch import Sources2DBatch
    from cnmf_e_amd.engine import Engine
    from cnmf_e_amd.sources2d import PatchedVideo, Sources2D
    c = bc.GROW
    d1, d2 = c["dims"]
    d = d1 * d2
    f, Y = bc.make_grow()
    opts = bc.grow_options(deconv=True)
    truth = np.asarray(f.A_true[:, [c["late"]]].todense()).ravel()
    ctr = bc.grow_centre()
    bat = []
    try:
        for t0, t1 in bc.ranges():
            eng = Engine(0)
            try:
                video = PatchedVideo(d1, d2, t1 - t0, [d1, d2], c["r"], eng)
                video.upload_from_full(Y[t0:t1])
                s = Sources2D(video, opts, sp.csc_matrix((d, 0), dtype=np.float32), np.zeros((0, t1 - t0), np.float32), np.zeros(d, np.float32))
                s.estimate_noise()
            except Exception:
                eng.close()
                raise
            bat.append(s)
        rec = []

        def watch(s):
            orig = s.initComponents_residual_parallel

            def wrapped(*a, **k):
                K0 = s.A.shape[1]
                center, _cn, _pnr = orig(*a, **k)
                rec.append(dict(K_before=K0, K_after=s.A.shape[1], center=np.asarray(center).reshape(-1, 2)))
                return center, _cn, _pnr
            s.initComponents_residual_parallel = wrapped
        for s in bat:
            watch(s)
        b = Sources2DBatch(bat, opts)
        b.initComponents_batch()
        K = b.A.shape[1]

        def corr_with_truth(A, k):
            return float(np.corrcoef(np.asarray(A[:, [k]].todense()).ravel(), truth)[0, 1])
        print("K around the second passes:", [(r["K_before"], r["K_after"]) for r in rec], "second-pass centres of batch 2:", rec[1]["center"].tolist(), "truth", ctr)
        # batch 1, after both of its passes, holds no neuron like the late one
        K1 = rec[0]["K_after"]
        c1 = [corr_with_truth(b.A, k) for k in range(K1)]
        print("batch 1's neurons against the late footprint:", np.round(c1, 3).tolist())
        assert K1 > 0 and max(c1) < 0.5
        # batch 2's SECOND pass finds it
        dist = np.hypot(rec[1]["center"][:, 0] - ctr[0], rec[1]["center"][:, 1] - ctr[1]) if rec[1]["center"].size else np.zeros(0)
        assert dist.size and dist.min() <= 3, (rec[1]["center"].tolist(), ctr)
        k_new = rec[1]["K_before"] + int(np.argmin(dist))
        assert rec[1]["K_before"] == K1 and k_new >= K1
        # afterwards every batch has the same K and the ids continue from P.k_ids
        assert [s.A.shape[1] for s in bat] == [K] * 3 and [s.C.shape[0] for s in bat] == [K] * 3 and K == rec[2]["K_after"]
        assert np.array_equal(b.ids, np.arange(1, K + 1)) and b.P["k_ids"] == K
        for s in bat:
            assert np.array_equal(s.ids, b.ids) and s.P["k_ids"] == K and len(s.tags) == K and np.array_equal(s.A.toarray(), b.A.toarray())
        # the new footprint is the late neuron's; its trace in batch 1, where it was silent, stays below that batch's noise level
        r_new = corr_with_truth(b.A, k_new)
        C1 = np.asarray(bat[0].C, dtype=np.float64)[k_new]
        sn1 = float(np.asarray(bat[0].P["neuron_sn"], dtype=np.float64).ravel()[k_new])
        C2 = np.asarray(bat[1].C, dtype=np.float64)[k_new]
        print("late neuron: column %d, footprint correlation %.3f, batch 1 max|C| %.6g against 3 x neuron_sn = %.6g; batch 2 max C %.3g" % (k_new, r_new, np.abs(C1).max(), 3 * sn1, C2.max()))
        assert r_new > 0.8
        assert np.abs(C1).max() < 3 * sn1
    finally:
        _close(bat)


# ---- 6. the demo's sequence ----------------------------------------------------------------------------------------------------------------------------------
def test_demo_sequence_three_live_contexts():
    from cnmf_e_amd.batch import Sources2DBatch
    cfg = CONFIGS["deconv"]
    bat, opts = _make_batches(cfg)
    try:
        b = Sources2DBatch(bat, opts)
        b.initComponents_batch()                                              # demo_batch_1p.m:123
        b.update_spatial_batch()                                              # :126
        b.update_temporal_batch()                                             # :129
        b.update_background_batch()                                           # :132
        pairs = b.correlation_pnr_batch()                                     # :139
        b.concatenate_temporal_batch()                                        # :142
        K = b.A.shape[1]
        assert K > 0 and b.C.shape == b.C_raw.shape == b.S.shape == (K, 304) and b.C.dtype == b.C_raw.dtype == b.S.dtype == np.float32
        for m, (t0, t1) in enumerate(bc.ranges()):
            for n in ("C", "C_raw", "S"):
                assert _same_bits(np.ascontiguousarray(getattr(b, n)[:, t0:t1]), np.array(getattr(bat[m], n), dtype=np.float32)), (m, n)
            Cn, PNR = bat[m].correlation_pnr_parallel()
            assert pairs[m][0].shape == (32, 32) and _same_bits(pairs[m][0], Cn) and _same_bits(pairs[m][1], PNR)
        assert np.isfinite(b.C).all() and np.isfinite(b.C_raw).all()
        # three contexts were alive throughout; they close in another order than they were made, and the others go on working
        bat[1].engine.close()
        bat[0].update_background_parallel()
        bat[2].engine.close()
        assert _same_bits(bat[0].engine.trace_energy(bat[0].C), bat[0]._trace_energy())
        bat[0].engine.close()
    finally:
        _close(bat)
