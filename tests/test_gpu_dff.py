"""extract_DF_F_endoscope on the engine (cnmfe.h section (i), csrc/dff.hpp) against tests/df_oracle.py.

1. the baselines in isolation, through df_load + df_finish: single order statistics bit-equal, averaged / interpolated ones within 8 * 2^-52 * max(|a|, |b|)
   (the rounding of a + (b - a) f with f itself a rounded quotient), the division (float)((double)C / Df) bit-equal where Df is, NaN rows for non-finite input;
   the long flavour (the trace read from global memory) against the LDS flavour and, at T = 24000 -- where 8 T bytes exceed a workgroup's 160 KB of LDS, so that
   ONLY the long flavour can run -- against the oracle by the same rules
2. the product alone: Yf of extract_DF_F_endoscope() against the oracle fed the ENGINE'S OWN reconstruct_background() in float64
3. end to end against the oracle's reconstruct_background() with the engine's A, C, C_raw
4. lanes = 2 and a one-rank RCCL group with force_collectives: bits of the plain run; no K x T upload after a deconvolving temporal update
5. refusals: every bad call comes back as an error code before anything is launched, and the context still works afterwards

Observed on MI355X (bounds = 10 x observed, rounded up to one digit):
  product, max |Yf - ref| / max |Yf|: 1.15e-15 (bg_ssub = 1), 1.09e-15 (bg_ssub = 2), 9.5e-16 / 1.09e-15 from a given Ybg     -> BOUND_PRODUCT = 2e-14
  end to end, relative to the largest entry: Df 6.9e-9 .. 1.9e-8, C_df and C_raw_df 5.75e-8 (the float32 rounding of the quotient)  -> BOUND_E2E = 6e-7"""
import os
import subprocess
import sys

import numpy as np
import pytest
import scipy.sparse as sp

import df_cases
import df_oracle

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

EPS = 2.0 ** -52
BOUND_PRODUCT = 2e-14        # 10 x the observed 1.15e-15, one digit up (fp64 sums of exact fp32 x fp32 products; anything above 1e-10 would mean fp32 arithmetic in the sum)
BOUND_E2E = 6e-7             # 10 x the observed 5.75e-8, one digit up (Ybg itself agrees with the oracle's to 5e-7: test_reconstruct_background_parity)


@pytest.fixture(scope="module")
def eng():
    from cnmf_e_amd.engine import Engine
    e = Engine(0)
    yield e
    e.close()


# ---- 1. the baselines in isolation ---------------------------------------------------------------------------------------------------
def _rows(T, seed=0):
    rng = np.random.default_rng(seed)
    g = rng.standard_normal(T) * 9 + 250
    q = rng.standard_normal(T)
    q = 250 + 5 * np.clip(np.round(q * 2), -4, 3)                          # eight levels: ties
    nan_row = rng.standard_normal(T) + 100
    nan_row[T // 3] = np.nan
    Yf = np.stack([g, q, np.full(T, 123.456), np.linspace(50.0, 90.0, T), nan_row, np.zeros(T)])
    inv = np.ones(6)
    inv[5] = np.inf                                                        # an empty footprint: 0 * Inf
    return Yf, inv


def _settings(T):
    return [(50, 0), (20, 0), (0, 0), (100, 0), (50, T + 5), (50, T), (30, T), (50, 51), (50, 50), (50, 1), (20, 51), (9, 50), (0.5, 50), (99.9, 50), (20, 2)]


def _check_against_oracle(Yf, got, C, R, p, w):
    """got = (C_df, C_raw_df, Df) of the engine for the scaled rows Yf"""
    C_df, R_df, Df = got
    Dfo, a, b = df_oracle.baseline(Yf, p, w or None, pairs=True)
    assert Df.shape == Dfo.shape
    single = (a == b)
    assert np.array_equal(Df[single], Dfo[single]), (p, w)
    two = ~single & np.isfinite(Dfo)
    assert np.all(np.abs(Df[two] - Dfo[two]) <= 8 * EPS * np.maximum(np.abs(a[two]), np.abs(b[two]))), (p, w, np.abs(Df[two] - Dfo[two]).max())
    assert np.array_equal(np.isnan(Df), np.isnan(Dfo))
    same = (Df == Dfo)
    for X, X_df in ((C, C_df), (R, R_df)):
        ref = df_oracle.divide(X, Dfo)
        m = same[:, None] & np.ones_like(ref, dtype=bool) if Df.ndim == 1 else same
        assert np.array_equal(X_df[m], ref[m]), (p, w)
        bad = np.isnan(Dfo)[:, None] & np.ones_like(ref, dtype=bool) if Df.ndim == 1 else np.isnan(Dfo)
        assert np.all(np.isnan(X_df[bad]))
    return int(single.sum()), int(two.sum())


@pytest.mark.parametrize("T", [403, 404])
def test_baselines_in_isolation(eng, T):
    Yf, inv = _rows(T)
    rng = np.random.default_rng(1)
    C = (rng.random((6, T)) * 40).astype(np.float32)
    R = (C + rng.standard_normal((6, T)).astype(np.float32)).astype(np.float32)
    with np.errstate(invalid="ignore"):
        Ys = Yf * inv[:, None]
    seen_two = 0
    for p, w in _settings(T):
        eng.df_load(Yf)
        C_df, R_df, Df, Yf_out = eng.df_finish(inv, p, w, C, R, want_Yf=True)
        assert np.array_equal(Yf_out, Ys, equal_nan=True)
        assert Df.shape == ((6, T) if 0 < w <= T else (6,))
        n1, n2 = _check_against_oracle(Ys, (C_df, R_df, Df), C, R, p, w)
        seen_two += n2
        assert np.all(np.isnan(Df[4:])) and np.all(np.isnan(C_df[4:])) and np.all(np.isnan(R_df[4:]))
        if (p, w) in ((0, 0), (100, 0), (50, 1), (9, 50), (0.5, 50), (99.9, 50), (20, 2)) or (p == 50 and (w == 0 or w > T) and T % 2):
            assert n2 == 0 and n1 > 0                                      # clamps, integer pt, odd-count medians: single order statistics, compared bit for bit
    assert seen_two > 0


def test_long_flavour_equals_the_lds_flavour(eng):
    """option trace_long = 1 at T = 403: the baseline kernels read the trace where it lies -- the same selections on the same keys, equal bits"""
    T = 403
    Yf, inv = _rows(T, seed=4)
    C = np.random.default_rng(2).random((6, T)).astype(np.float32)
    outs = {}
    for lng in (0, 1):
        eng.set_option("trace_long", lng)
        try:
            outs[lng] = []
            for p, w in [(50, 0), (20, 0), (50, 51), (50, 50), (20, 51), (9, 50)]:
                eng.df_load(Yf)
                outs[lng].append(eng.df_finish(inv, p, w, C, C))
        finally:
            eng.set_option("trace_long", 0)
    for a, b in zip(outs[0], outs[1]):
        for x, y in zip(a, b):
            assert np.array_equal(x, y, equal_nan=True)


def test_a_trace_beyond_lds(eng):
    """T = 24000, K = 3, w = 1001: 8 T bytes do not fit a workgroup's LDS, the windowed median reads the accumulator row in global memory; windows in the
    interior hold 1001 samples (a single order statistic: bit-equal), the clipped ones at the ends an even count now and then (the 8-ulp bound)"""
    T, K, w = 24000, 3, 1001
    rng = np.random.default_rng(8)
    Yf = np.cumsum(rng.standard_normal((K, T)), axis=1) + 400
    inv = np.ones(K)
    C = rng.random((K, T)).astype(np.float32)
    eng.df_load(Yf)
    C_df, R_df, Df = eng.df_finish(inv, 50, w, C, C)
    from numpy.lib.stride_tricks import sliding_window_view
    h = (w - 1) // 2
    ref = np.empty((K, T)); a = np.empty((K, T)); b = np.empty((K, T))
    ref[:, h:T - h] = np.median(sliding_window_view(Yf, w, axis=1), axis=2)
    a[:, h:T - h] = b[:, h:T - h] = ref[:, h:T - h]
    for k in range(K):
        for t in list(range(h)) + list(range(T - h, T)):
            s = np.sort(Yf[k, max(t - h, 0):min(t + h, T - 1) + 1])
            a[k, t], b[k, t] = s[(s.size - 1) // 2], s[s.size // 2]
            ref[k, t] = a[k, t] if s.size % 2 else 0.5 * (a[k, t] + b[k, t])
    single = a == b
    assert np.array_equal(Df[single], ref[single])
    assert np.all(np.abs(Df - ref) <= 8 * EPS * np.maximum(np.abs(a), np.abs(b)))
    assert np.array_equal(C_df[single], df_oracle.divide(C, ref)[single])
    eng.df_load(Yf)                                                        # the global baseline of the same rows: select_pair64 on the row in global memory
    _, _, Df_g = eng.df_finish(inv, 20, 0, C, C)
    assert np.all(np.abs(Df_g - df_oracle.baseline(Yf, 20, None)) <= 8 * EPS * np.abs(Yf).max())


# ---- 2. / 3. the product and the whole call on a recording ------------------------------------------------------------------------------
class _State:
    """the recording of tests/df_cases.py after one iteration, on the engine"""

    def __init__(self, eng, bg_ssub=1, lanes=1, **opts):
        from cnmf_e_amd.sources2d import PatchedVideo, Sources2D, Options
        self.f, self.Y = df_cases.recording()
        r = df_cases.radius(bg_ssub)
        if lanes > 1:
            eng.set_option("lanes", lanes)
        video = PatchedVideo(df_cases.D1, df_cases.D2, df_cases.T, df_cases.PATCH, r, eng)
        video.upload_from_full(self.Y)
        self.s = Sources2D(video, Options(ring_radius=r, maxIter=3, bg_ssub=bg_ssub, **opts), self.f.A_init, self.f.C_init, self.f.sn)
        for step in ("update_background_parallel", "update_spatial_parallel", "update_temporal_parallel"):
            getattr(self.s, step)()


def _fresh_engine():
    from cnmf_e_amd.engine import Engine
    return Engine(0)


@pytest.mark.parametrize("bg_ssub", [1, 2])
def test_product_against_the_engines_own_background(bg_ssub, observed):
    e = _fresh_engine()
    try:
        s = _State(e, bg_ssub).s
        Ybg = s.reconstruct_background().astype(np.float64).reshape(df_cases.D1 * df_cases.D2, df_cases.T, order="F")
        ref = df_oracle.project(s.A, Ybg)
        assert max(len(x) for x in df_cases.patches_of_neurons(sp.csc_matrix(s.A))) >= 2       # the accumulation crosses patches
        out1 = s.extract_DF_F_endoscope(want_Yf=True)
        err = np.abs(out1[3] - ref).max() / np.abs(ref).max()
        print("product bg_ssub=%d: max |Yf - ref| / max |Yf| = %.3e" % (bg_ssub, err))
        observed["dff_product_ssub%d" % bg_ssub] = float(err)
        assert err <= BOUND_PRODUCT, err
        out2 = s.extract_DF_F_endoscope(want_Yf=True)
        for x, y in zip(out1, out2):
            assert np.array_equal(x, y)                                    # two calls: equal bits
        out3 = s.extract_DF_F_endoscope(Ybg=s.reconstruct_background(), want_Yf=True)
        err3 = np.abs(out3[3] - ref).max() / np.abs(ref).max()
        print("product from a given Ybg: %.3e" % err3)
        observed["dff_product_given_ssub%d" % bg_ssub] = float(err3)
        assert err3 <= BOUND_PRODUCT, err3
        assert out1[2].shape == (df_cases.K,) and out1[0].dtype == np.float32 and out1[0].shape == np.asarray(s.C).shape
    finally:
        e.close()


def test_end_to_end_against_the_oracle(observed):
    e = _fresh_engine()
    try:
        st = _State(e)
        s = st.s
        o = df_cases.oracle_after_one_iteration(st.f, st.Y)
        o.A = s.A.astype(np.float64); o.C = np.asarray(s.C, dtype=np.float64)   # same model on both sides (as test_init_residual_parity does)
        for idx in s.video.owned:
            o.W[idx] = s.get_W(idx).astype(np.float64); o.b0[idx] = np.asarray(s.get_b0(idx), dtype=np.float64)
        Ybg = o.reconstruct_background()
        worst = 0.0
        for p, w in df_cases.E2E_SETTINGS:
            s.options.df_prctile, s.options.df_window = p, w
            C_df, R_df, Df = s.extract_DF_F_endoscope()
            rC, rR, rD = df_oracle.extract_df_f(s.A, np.asarray(s.C), np.asarray(s.C_raw), Ybg, p, w)
            assert Df.shape == rD.shape and Df.dtype == np.float64 and C_df.dtype == np.float32
            errs = [np.abs(Df - rD).max() / np.abs(rD).max(), np.abs(C_df - rC).max() / np.abs(rC).max(), np.abs(R_df - rR).max() / np.abs(rR).max()]
            print("end to end (p, w) = (%s, %s): Df %.3e  C_df %.3e  C_raw_df %.3e" % (p, w, *errs))
            observed["dff_e2e_p%s_w%s" % (p, w)] = [float(x) for x in errs]
            worst = max(worst, *errs)
        assert worst <= BOUND_E2E, worst
    finally:
        e.close()


# ---- 4. lanes, collectives, uploads -----------------------------------------------------------------------------------------------------
def test_two_lanes_give_the_bits_of_one():
    outs = []
    for lanes in (1, 2):
        e = _fresh_engine()
        try:
            s = _State(e, lanes=lanes, df_prctile=20, df_window=50).s
            outs.append(s.extract_DF_F_endoscope(want_Yf=True))
        finally:
            e.close()
    for x, y in zip(*outs):
        assert np.array_equal(x, y)


def test_forced_collectives_on_an_rccl_group():
    """one rank of an nccl group with force_collectives: df_fetch, the all-reduce, df_load -- the bits of the unsharded run (scripts/df_nccl_smoke.py, in its own
    process: it owns a process group)"""
    env = dict(os.environ, MASTER_ADDR="127.0.0.1", MASTER_PORT="29547", HSA_ENABLE_IPC_MODE_LEGACY="0")
    out = subprocess.run([sys.executable, os.path.join(ROOT, "scripts", "df_nccl_smoke.py")], capture_output=True, text=True, timeout=300, env=env)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
    assert "dF/F forced collectives: equal bits" in out.stdout


def test_no_trace_upload_after_a_deconvolving_update():
    e = _fresh_engine()
    try:
        s = _State(e, deconv_flag=True).s
        before = e.counter("merge_trace_uploads")
        C_df, R_df, Df = s.extract_DF_F_endoscope()
        assert e.counter("merge_trace_uploads") == before
        assert np.array_equal(C_df, df_oracle.divide(np.asarray(s.C), Df)) and np.array_equal(R_df, df_oracle.divide(np.asarray(s.C_raw), Df))
    finally:
        e.close()


# ---- 5. refusals -----------------------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_context_usable():
    from cnmf_e_amd._lib import CnmfeError
    e = _fresh_engine()
    try:
        st = _State(e)
        s, v = st.s, st.s.video
        K, T = np.asarray(s.C).shape
        idx = v.owned[0]
        pid, d = v.pid[idx], v.patch_pix[idx].size
        A1 = sp.csc_matrix((np.ones(2, np.float32), np.array([0, d - 1]), np.array([0, 1, 2])), shape=(d, 2))
        b0b, b0n = np.zeros(v.block_pix[idx].size, np.float32), np.zeros(d, np.float32)
        Yb = np.zeros((8, d), np.float32)

        def refused(code, fn, *a):
            with pytest.raises(CnmfeError, match="error %d" % code):
                fn(*a)

        refused(-4, e.df_add_frames, Yb, 0, A1, [0, 1])                    # no df_begin
        refused(-4, e.df_add_background, pid, b0b, b0n, A1, [0, 1])
        e.df_begin(K, T)
        refused(-4, e.df_begin, K, T)                                      # a second begin
        # a row index = d: built by hand, scipy would refuse the matrix
        import ctypes as C
        from cnmf_e_amd import _lib as L
        cp, ri, va = np.array([0, 1, 2], np.int64), np.array([0, d], np.int32), np.ones(2, np.float32)
        ind = np.array([0, 1], np.int32)
        ptr = lambda a, t: a.ctypes.data_as(t)
        rc = L.lib.cnmfe_df_add_frames(e._ctx, d, 0, 8, Yb.ctypes.data_as(C.c_void_p), L.HOST, 2, ptr(cp, L.i64p), ptr(ri, L.i32p), ptr(va, L.f32p), ptr(ind, L.i32p))
        assert rc == -1
        rc = L.lib.cnmfe_df_add_background(e._ctx, pid, ptr(b0b, L.f32p), ptr(b0n, L.f32p), 2, ptr(cp, L.i64p), ptr(ri, L.i32p), ptr(va, L.f32p), ptr(ind, L.i32p))
        assert rc == -1
        refused(-1, e.df_add_frames, Yb, 0, A1, [1, 1])                    # a repeated accumulator row
        refused(-1, e.df_add_frames, Yb, 0, A1, [0, K])                    # a row outside the accumulator
        refused(-1, e.df_add_frames, Yb, T - 7, A1, [0, 1])                # frame0 + nframes > T
        refused(-1, e.df_finish, np.ones(K), 101, 0, np.asarray(s.C), np.asarray(s.C))
        e.df_close()
        # a patch without a residual: a fresh engine state for that patch
        e2 = _fresh_engine()
        try:
            from cnmf_e_amd.sources2d import PatchedVideo
            v2 = PatchedVideo(df_cases.D1, df_cases.D2, df_cases.T, df_cases.PATCH, 5, e2)
            v2.upload_from_full(st.Y)
            for i2 in v2.owned:
                e2.ring_init(v2.pid[i2], 5)
            e2.df_begin(K, T)
            refused(-4, e2.df_add_background, v2.pid[idx], b0b, b0n, A1, [0, 1])
            e2.df_close()
        finally:
            e2.close()
        # after all of it a complete begin .. finish sequence still works, and gives what it gave before
        ref = s.extract_DF_F_endoscope(want_Yf=True)
        e.df_begin(K, T)
        refused(-1, e.df_add_frames, Yb, 0, A1, [1, 1])
        e.df_close()
        again = s.extract_DF_F_endoscope(want_Yf=True)
        for x, y in zip(ref, again):
            assert np.array_equal(x, y)
    finally:
        e.close()
