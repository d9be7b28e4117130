"""CPU tests of the closing calls (orderROIs, demixed_frames, show_demixed_video): the oracle's self-checks, the product's host rules (cnmf_e_amd/hostops.py)
against tests/demix_oracle.py, the fixture of tests/demix_cases.py, and Sources2D's three methods over an engine double -- argument marshalling, chunking,
refusals, the TIFF."""
import os

import numpy as np
import pytest
import scipy.sparse as sp

import demix_cases as dc
import demix_oracle as do
from cnmf_e_amd import hostops
from fake_engine import FakeEngine


# ---- the oracle itself -----------------------------------------------------------------------------------------------------------------
def test_uint16_conversion():
    x = np.array([-0.5, 0.5, 65535.5, np.nan, 0.49999, 1.5, 2.5, -3.0, 65534.5, 1e9, np.inf, -np.inf])
    want = np.array([0, 1, 65535, 0, 0, 2, 3, 0, 65535, 65535, 65535, 0], dtype=np.uint16)
    assert np.array_equal(do.matlab_uint16(x), want)
    assert np.array_equal(hostops.matlab_uint16(x), want)
    rng = np.random.default_rng(0)
    y = np.concatenate([rng.random(2000) * 70000 - 2000, np.arange(0, 50) + 0.5])
    assert np.array_equal(hostops.matlab_uint16(y), do.matlab_uint16(y))


def test_panel_identities():
    rng = np.random.default_rng(1)
    d, n, K = 30, 7, 4
    raw, bg = rng.random((d, n)) * 100, rng.random((d, n)) * 90
    A = sp.random(d, K, density=0.3, random_state=2, format="csc")
    CC, col = rng.random((K, n)) * 5, rng.random((K, 3))
    p = do.panels_from(raw, bg, A, CC, col, 3.0)
    assert np.array_equal(p["signal"], raw - bg) and np.array_equal(p["residual"], p["signal"] - p["denoised"])
    assert np.allclose(p["denoised"], A.toarray() @ CC)
    one = do.panels_from(raw, bg, A, CC, np.ones((K, 3)), 3.0)              # white neurons: every colour plane is the denoised panel, scaled
    for m in range(3):
        assert np.allclose(one["mixed_double"][:, :, m], p["denoised"] * 2 / 3.0 * 65536)
    none = do.panels_from(raw, bg, sp.csc_matrix((d, 0)), np.zeros((0, n)), np.zeros((0, 3)), 3.0)
    assert not none["denoised"].any() and not none["mixed"].any() and np.array_equal(none["residual"], raw - bg)
    assert np.array_equal(do.rounding_distance([0.5, 1.0, 1.45, -1.0, 70000.0]) < 0.051, [True, False, True, False, False])


@pytest.mark.parametrize("descend", [False, True])
def test_matlab_sort_order_against_a_brute_force_stable_sort(descend):
    rng = np.random.default_rng(3)
    for trial in range(40):
        n = int(rng.integers(0, 12))
        x = rng.integers(0, 4, size=n).astype(np.float64)                    # many ties
        x[rng.random(n) < 0.25] = np.nan
        if n > 2 and trial % 3 == 0:
            x[0], x[-1] = np.inf, -np.inf
        assert np.array_equal(hostops.matlab_sort_order(x, descend=descend), do.stable_sort_brute(x, descend)), (x, descend)
    x = np.array([2.0, np.nan, 2.0, 5.0, np.nan, 1.0])
    assert hostops.matlab_sort_order(x).tolist() == [5, 0, 2, 3, 1, 4]                    # ascend: NaN last, ties in order
    assert hostops.matlab_sort_order(x, descend=True).tolist() == [1, 4, 3, 0, 2, 5]      # descend: NaN first, ties in order


def test_ranges_follow_the_reference():
    rng = np.random.default_rng(4)
    raw = rng.random(5000) * 300 + 100
    for kw in (dict(), dict(multi_factor=7.0), dict(range_Y=[90.0, 400.0]), dict(range_Y=[90.0, 400.0], multi_factor=3.0), dict(range_ac=[1.0, 50.0])):
        got = hostops.demix_ranges(40.0, raw, **kw)
        ref = do.ranges(40.0, raw, quantile=hostops.matlab_quantile, **kw)
        for k in ("range_ac", "range_res", "range_Y", "multi_factor"):
            assert np.allclose(got[k], ref[k], rtol=1e-14, atol=0), (kw, k)
    r = hostops.demix_ranges(40.0, raw)
    assert np.allclose(r["range_ac"], [0.4, 40.4]) and np.isclose(r["range_res"].sum(), 0) and r["multi_factor"] == np.ceil(np.diff(hostops.matlab_quantile(raw, [0.01, 0.98]))[0] / 40.0)
    with pytest.raises(ValueError):
        hostops.demix_ranges(40.0)


def test_imagesc_and_montage():
    v = np.array([[-1.0, 0.0, 0.5], [0.999, 1.0, np.nan]])
    assert hostops.imagesc_8bit(v, 0.0, 1.0).tolist() == [[0, 0, 128], [255, 255, 0]]
    d1, d2 = 4, 5
    fr = {k: np.full((d1, d2), i, dtype=np.float32) for i, k in enumerate(("raw", "bg", "signal", "denoised", "residual"))}
    fr["mixed"] = np.full((d1, d2, 3), 0x1234, dtype=np.uint16)
    rg = dict(range_Y=np.array([0.0, 2.0]), range_ac=np.array([0.0, 4.0]), range_res=np.array([0.0, 8.0]))
    img = hostops.demixed_montage(fr, rg)
    assert img.shape == (2 * d1, 3 * d2, 3) and img.dtype == np.uint8
    tiles = [[img[:d1, j * d2:(j + 1) * d2] for j in range(3)], [img[d1:, j * d2:(j + 1) * d2] for j in range(3)]]
    assert [int(t[0, 0, 0]) for t in tiles[0]] == [0, 128, 128]             # raw (0 of [0, 2]), raw - bg (2 of [0, 4]), residual (4 of [0, 8])
    assert [int(t[0, 0, 0]) for t in tiles[1]] == [128, 192, 0x12]          # bg (1 of [0, 2]), denoised (3 of [0, 4]), the demixed panel's high byte
    assert hostops.prism64().shape == (64, 3) and np.array_equal(hostops.prism64()[6], [1.0, 0.0, 0.0])


# ---- the fixture -----------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def states():
    return {False: dc.oracle_state(1, deconv=False), True: dc.oracle_state(1, deconv=True)}


def test_fixture_mixed_samples_are_away_from_rounding_boundaries(states):
    """the exactness clause of the GPU panel test covers almost all samples: fewer than 2 % of the oracle's mixed samples lie within MIXED_MARGIN of a boundary"""
    f, Y, o = states[False]
    md = do.mixed_double(o.A, o.C[:, dc.frames()], dc.colors(dc.K), dc.AMP_AC)
    frac = float((do.rounding_distance(md) <= dc.MIXED_MARGIN).mean())
    lit = float(((md > 0.5) & (md < 65535.5)).mean())
    print("mixed samples within %.2f of a rounding boundary: %.4f; lit and unsaturated: %.4f" % (dc.MIXED_MARGIN, frac, lit))
    assert frac < 0.02, frac
    assert lit > 0.02, lit                                                   # (and the panel is not all black or all saturated)


def test_fixture_order_margins(states):
    """neighbouring SNR / PNR values of the deconvolved state differ by more than ORDER_MARGIN relative: the engine's fp64 statistics give the oracle's order"""
    f, Y, o = states[True]
    for name in ("snr", "pnr", "sparsity_temporal", "mean"):
        srt, val = do.order_rois(name, o.A, o.C, o.C_raw)
        assert np.all(np.isfinite(val)), name
        assert do.margin(val) > dc.ORDER_MARGIN, (name, do.margin(val))
        assert sorted(srt.tolist()) == list(range(dc.K))
    C, R = dc.tie_nan_traces()
    srt, val = do.order_rois("snr", o.A, C, R)
    assert np.isnan(val[2]) and np.isinf(val[5]) and val[1] == val[4]
    assert srt[0] == 2 and srt[1] == 5 and list(srt).index(1) + 1 == list(srt).index(4)      # NaN first, then Inf; the tie in its order
    rest = np.delete(val, [2, 4, 5])
    assert do.margin(rest) > dc.ORDER_MARGIN


def test_fixture_halo_neuron_has_an_empty_patch_column():
    from cnmf_e_amd.sources2d import PatchedVideo
    from test_gpu_mex_gateway import _Geometry
    geo = PatchedVideo(dc.D1, dc.D2, dc.T, dc.PATCH, dc.radius(1), _Geometry())
    a, c = dc.halo_neuron()
    idx = geo.order[0]
    assert a[geo.block_pix[idx]].nnz == a.nnz == 9 and a[geo.patch_pix[idx]].nnz == 0 and c.shape == (dc.T,)


# ---- Sources2D over an engine double ---------------------------------------------------------------------------------------------------
class DemixFake(FakeEngine):
    """FakeEngine + the calls the closing methods make, in float64 NumPy, every call recorded"""
    supports_bound_traces = True

    def __init__(self):
        super().__init__()
        self.calls = []
        self._bound = None
        self._res = None
        self.uploads = 0

    def bind_traces(self, Cm, device_ptr=None):
        self._bound = Cm
        self._res = None

    def residents_are(self, Cm, C_raw, S):
        r = self._res
        return r is not None and Cm is r[0] and C_raw is r[1] and S is r[2]

    def traces_load(self, Cm, C_raw=None, S=None, kernel_pars=None):
        self.uploads += 1
        self._bound = Cm
        self._res = (Cm, Cm if C_raw is None else C_raw, S)
        self._kp = None if kernel_pars is None else np.asarray(kernel_pars, dtype=np.float32)

    def trace_order_stats(self):
        self.calls.append(("trace_order_stats",))
        return do.order_stats(self._res[0], self._res[1])

    def merge_apply(self, groups, weights, keep, deconv_options=None):
        assert groups == [] and weights == []
        self.calls.append(("merge_apply", np.asarray(keep).tolist()))
        keep = np.asarray(keep)
        Cn, Rn = np.asarray(self._res[0])[keep], np.asarray(self._res[1])[keep]
        Sn = None if self._res[2] is None else np.asarray(self._res[2])[keep]
        kp = np.zeros(keep.size, np.float32) if self._kp is None else self._kp[keep]
        self._bound, self._res, self._kp = Cn, (Cn, Rn, Sn), kp
        return Cn, Rn, Sn, kp, np.zeros(keep.size, np.float32)

    def reconstruct_background(self, pid, b0_block, b0_new_patch, frame0=0, nframes=None):
        q = self.p[pid]
        R = q["Y"].T.astype(np.float64) - np.asarray(b0_block, dtype=np.float64)[:, None]
        Ap, Cp = q.get("res_AC", (None, None))
        if Ap is not None and Ap.shape[1]:
            R = R - Ap @ Cp
        return (q["W"] @ R + np.asarray(b0_new_patch, dtype=np.float64)[:, None])[:, frame0:frame0 + nframes].T

    def demix_frames(self, pid, b0_block, b0_new_patch, A_patch, CC, ind, col, mix_scale, frame0, stride, nframes, want=None):
        self.calls.append(("demix_frames", pid, int(frame0), int(stride), int(nframes), np.asarray(ind).tolist(), CC is self._bound, float(mix_scale)))
        q = self.p[pid]
        if frame0 < 0 or stride < 1 or nframes < 0 or (nframes and frame0 + (nframes - 1) * stride >= q["T"]):
            raise RuntimeError("cnmfe error -1")
        t = frame0 + stride * np.arange(nframes)
        raw = q["Y"].T.astype(np.float64)[q["ip"]][:, t]
        bg = self.reconstruct_background(pid, b0_block, b0_new_patch, 0, q["T"]).T[:, t]
        K = 0 if A_patch is None else A_patch.shape[1]
        A = sp.csc_matrix((raw.shape[0], 0)) if K == 0 else A_patch
        p = do.panels_from(raw, bg, A, np.asarray(CC, dtype=np.float64)[np.asarray(ind, dtype=np.int64)][:, t], np.asarray(col).reshape(-1, 3), 2.0 * 65536.0 / mix_scale if K else 1.0)
        out = {k: p[k].T.astype(np.float32) for k in ("raw", "bg", "signal", "denoised", "residual")}
        out["mixed"] = np.ascontiguousarray(p["mixed"].transpose(2, 1, 0))
        return out


@pytest.fixture(scope="module")
def host(states):
    """a Sources2D over the double, holding the oracle's state after one iteration (no deconvolution)"""
    from cnmf_e_amd.sources2d import PatchedVideo, Sources2D, Options
    f, Y, o = states[False]
    eng = DemixFake()
    video = PatchedVideo(dc.D1, dc.D2, dc.T, dc.PATCH, dc.radius(1), eng)
    video.upload_from_full(Y)
    s = Sources2D(video, Options(ring_radius=dc.radius(1), maxIter=3), f.A_init, f.C_init, f.sn)
    for step in ("update_background_parallel", "update_spatial_parallel", "update_temporal_parallel"):
        getattr(s, step)()
    return s, eng, o, Y


def _oracle_like(s, o):
    """the oracle holding the double's model: the expression is what is compared"""
    import copy
    o2 = copy.copy(o)
    o2.A, o2.C, o2.C_raw = sp.csc_matrix(s.A).astype(np.float64), np.asarray(s.C, dtype=np.float64), np.asarray(s.C_raw, dtype=np.float64)
    o2.A_prev, o2.C_prev = sp.csc_matrix(s.A_prev).astype(np.float64), np.asarray(s.C_prev, dtype=np.float64)
    o2.W = {idx: s.get_W(idx).astype(np.float64) for idx in s.video.owned}
    o2.b0 = {idx: np.asarray(s.get_b0(idx), dtype=np.float64) for idx in s.video.owned}
    o2.b0_new = np.asarray(s.b0_new, dtype=np.float64)
    return o2


def test_demixed_frames_chunks_and_panels(host):
    s, eng, o, Y = host
    K = s.A.shape[1]
    col = dc.colors(K)
    o2 = _oracle_like(s, o)
    Ybg = o2.reconstruct_background()
    # kt = 1: 100 + 100 + 3 displayed frames
    eng.calls.clear()
    chunks = list(s.demixed_frames(amp_ac=dc.AMP_AC, colors=col))
    assert [c["frames"].size for c in chunks] == [100, 100, 3]
    assert np.array_equal(np.concatenate([c["frames"] for c in chunks]), np.arange(1, dc.T + 1))
    calls = [c for c in eng.calls if c[0] == "demix_frames"]
    npatch = len(s.video.owned)
    assert len(calls) == 3 * npatch
    assert [(c[2], c[3], c[4]) for c in calls[::npatch]] == [(0, 1, 100), (100, 1, 100), (200, 1, 3)]
    assert all(np.isclose(c[7], 2.0 / dc.AMP_AC * 65536.0, rtol=1e-15) for c in calls)                        # mix_scale
    assert chunks[0]["raw"].shape == (dc.D1, dc.D2, 100) and chunks[2]["mixed"].shape == (dc.D1, dc.D2, 3, 3) and chunks[0]["mixed"].dtype == np.uint16
    ref = do.panels(o2, np.arange(dc.T), o2.C, col, dc.AMP_AC, Ybg=Ybg)
    for name in ("raw", "bg", "signal", "denoised", "residual"):
        got = np.concatenate([c[name] for c in chunks], axis=2).reshape(dc.D1 * dc.D2, dc.T, order="F")
        # (b0 crosses the interface as float32 and the double returns float32: a few roundings at the scale of the raw video, whatever the panel's own scale)
        assert np.abs(got - ref[name]).max() <= 1e-6 * np.abs(ref["raw"]).max(), name
    got = np.concatenate([c["mixed"] for c in chunks], axis=2).reshape(dc.D1 * dc.D2, dc.T, 3, order="F")
    far = do.rounding_distance(ref["mixed_double"]) > 1e-6
    assert np.array_equal(got[far], ref["mixed"][far])
    # kt = 3 over (6, 203) with chunk = 25: 66 displayed frames = 25 + 25 + 16, each chunk starting where the last one ended
    eng.calls.clear()
    chunks = list(s.demixed_frames(kt=dc.KT, frame_range=dc.FRAME_RANGE, amp_ac=dc.AMP_AC, colors=col, use_craw=True, chunk=25))
    fr = np.concatenate([c["frames"] for c in chunks])
    assert np.array_equal(fr, dc.frames() + 1) and [c["frames"].size for c in chunks] == [25, 25, 16]
    calls = [c for c in eng.calls if c[0] == "demix_frames"]
    assert [(c[2], c[3], c[4]) for c in calls[::npatch]] == [(5, 3, 25), (80, 3, 25), (155, 3, 16)]
    ref = do.panels(o2, dc.frames(), o2.C_raw, col, dc.AMP_AC, Ybg=Ybg)
    got = np.concatenate([c["denoised"] for c in chunks], axis=2).reshape(dc.D1 * dc.D2, -1, order="F")
    assert np.abs(got - ref["denoised"]).max() <= 1e-5 * np.abs(ref["denoised"]).max()
    # every patch sees exactly the neurons with pixels on it
    for c in calls[:npatch]:
        idx = [i for i in s.video.owned if s.video.pid[i] == c[1]][0]
        want = np.flatnonzero(np.asarray(abs(sp.csc_matrix(s.A)[s.video.patch_pix[idx]]).sum(axis=0)).ravel() > 0)
        assert c[5] == want.tolist()


def test_demixed_frames_defaults_and_refusals(host):
    s, eng, o, Y = host
    K = s.A.shape[1]
    eng.calls.clear()
    ch = next(s.demixed_frames(frame_range=(10, 12)))
    amp = do.default_amp_ac(s.A, np.asarray(s.C))
    call = [c for c in eng.calls if c[0] == "demix_frames"][0]
    assert np.isclose(call[7], 2.0 / amp * 65536.0, rtol=1e-12) and ("trace_order_stats",) in eng.calls
    assert ch["frames"].tolist() == [10, 11, 12]
    col = hostops.prism64()[np.random.default_rng(0).integers(0, 64, size=K)]
    ref = next(s.demixed_frames(frame_range=(10, 12), colors=col))
    assert np.array_equal(ch["mixed"], ref["mixed"])                         # the default colours: prism(64) rows drawn by default_rng(0), once
    for bad in (dict(kt=0), dict(chunk=0), dict(frame_range=(0, 5)), dict(frame_range=(5, dc.T + 1)), dict(frame_range=(9, 3)), dict(colors=np.ones((K + 1, 3)))):
        with pytest.raises(ValueError):
            next(s.demixed_frames(**bad))


def test_show_demixed_video_writes_a_tiff(host, tmp_path):
    Image = pytest.importorskip("PIL.Image")
    s, eng, o, Y = host
    path = str(tmp_path / "demixed.tif")
    rg = s.show_demixed_video(path, kt=dc.KT, frame_range=(6, 60))
    n = len(range(6, 61, dc.KT))
    with Image.open(path) as im:
        assert im.n_frames == n and im.size == (3 * dc.D2, 2 * dc.D1) and im.mode == "RGB"
        im.seek(n - 1)
        last = np.array(im)
    ch = list(s.demixed_frames(kt=dc.KT, frame_range=(6, 60)))[-1]
    want = hostops.demixed_montage({k: ch[k][:, :, -1] for k in ("raw", "bg", "signal", "denoised", "residual", "mixed")}, rg)
    assert np.array_equal(last, want)
    first_raw = next(s.demixed_frames(kt=dc.KT, frame_range=(6, 60)))["raw"]
    ref = do.ranges(rg["amp_ac"], first_raw, quantile=hostops.matlab_quantile)
    assert np.allclose(rg["range_Y"], ref["range_Y"]) and rg["multi_factor"] == ref["multi_factor"]
    assert np.isclose(rg["amp_ac"], do.default_amp_ac(s.A, np.asarray(s.C)))
    given = s.show_demixed_video(None, frame_range=(1, 4), amp_ac=50.0, range_Y=[100.0, 300.0])      # nothing written; :54-57
    assert given["multi_factor"] == round(200.0 / 50.0) and not os.path.exists(str(tmp_path / "none.tif"))


def test_show_demixed_video_without_pil(host, monkeypatch):
    import builtins
    s = host[0]
    real = builtins.__import__

    def no_pil(name, *a, **k):
        if name == "PIL" or name.startswith("PIL."):
            raise ImportError("no PIL here")
        return real(name, *a, **k)
    monkeypatch.setattr(builtins, "__import__", no_pil)
    with pytest.raises(RuntimeError, match="PIL"):
        s.show_demixed_video("x.tif", frame_range=(1, 2))


def test_order_rois_over_the_double(states):
    from cnmf_e_amd.sources2d import PatchedVideo, Sources2D, Options
    f, Y, o = states[True]
    K = dc.K
    eng = DemixFake()
    video = PatchedVideo(dc.D1, dc.D2, dc.T, dc.PATCH, dc.radius(1), eng)
    video.upload_from_full(Y)
    s = Sources2D(video, Options(ring_radius=dc.radius(1), maxIter=3, deconv_flag=True), f.A_init, f.C_init, f.sn)
    A0 = sp.csc_matrix(o.A, dtype=np.float32)
    C0, R0 = o.C.astype(np.float32), o.C_raw.astype(np.float32)

    def fresh():
        s.set_components(A0, C0, R0)
        s.S = np.arange(K, dtype=np.float32)[:, None] * np.ones((1, dc.T), np.float32)
        s.P["kernel_pars"] = np.linspace(0.95, 0.5, K).astype(np.float32)
        s.P["neuron_sn"] = np.arange(1, K + 1, dtype=np.float32)
        s.ids, s.tags = np.arange(100, 100 + K), np.arange(K, dtype=np.uint16)
        eng.calls.clear()
    for name in ("snr", "srt", "anything else", "pnr", "PNR", "mean", "sparsity_spatial", "sparsity_temporal", "decay_time", "Decay_Time"):
        fresh()
        A_prev, C_prev = s.A_prev, s.C_prev
        srt = s.orderROIs(name)
        ref_name = name if name.lower() in ("pnr", "decay_time") or name in ("mean", "sparsity_spatial", "sparsity_temporal") else "snr"
        want, _ = do.order_rois(ref_name, A0, C0, R0, kernel_pars=np.linspace(0.95, 0.5, K).astype(np.float32))
        assert np.array_equal(srt, want), name
        assert ("merge_apply", want.tolist()) in eng.calls
        assert np.array_equal(s.A.toarray(), A0.toarray()[:, srt]) and np.array_equal(np.asarray(s.C), C0[srt]) and np.array_equal(np.asarray(s.C_raw), R0[srt])
        assert np.array_equal(s.S[:, 0], srt) and np.array_equal(s.ids, 100 + srt) and np.array_equal(s.tags, srt)
        assert np.array_equal(s.P["kernel_pars"], np.linspace(0.95, 0.5, K).astype(np.float32)[srt])
        assert s.A_prev is A_prev and s.C_prev is C_prev
    fresh()
    perm = np.array([3, 0, 5, 1, 4, 2])
    assert np.array_equal(s.orderROIs(perm), perm) and np.array_equal(np.asarray(s.C), C0[perm])
    assert ("trace_order_stats",) not in eng.calls
    for bad in ([0, 1, 2], [0, 1, 2, 3, 4, 4], [0, 1, 2, 3, 4, 6], [[0, 1, 2, 3, 4, 5]], np.arange(K) + 0.5):
        with pytest.raises(ValueError):
            s.orderROIs(bad)
    for name in ("circularity", "temporal_cluster", "Spatial_Cluster"):
        with pytest.raises(NotImplementedError):
            s.orderROIs(name)
    # 'mean' without deconv_flag reads P.neuron_sn
    fresh()
    s.options.deconv_flag = False
    try:
        want, _ = do.order_rois("mean", A0, C0, R0, deconv_flag=False, neuron_sn=np.arange(1, K + 1, dtype=np.float32))
        assert np.array_equal(s.orderROIs("mean"), want)
        fresh()
        del s.P["neuron_sn"]
        with pytest.raises(ValueError, match="neuron_sn"):
            s.orderROIs("mean")
    finally:
        s.options.deconv_flag = True
    # the tie and the NaN
    C, R = dc.tie_nan_traces()
    s.set_components(A0, C, R)
    want, _ = do.order_rois("snr", A0, C, R)
    assert np.array_equal(s.orderROIs("snr"), want) and want[0] == 2
