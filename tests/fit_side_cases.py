"""The runs of tests/test_gpu_fit_side.py and of scripts/make_fit_setup_golden.py (which recorded tests/golden/fit_setup_parent.npz with them, on the parent commit's
library): ring fits whose set-up takes every branch of bg_fit_ring that the kept geometry tables, the device-side sum(A, 2) / slot_of and option fit_side touch.
All on 48 x 48 patches with K = 8 seeded footprints (tests/solve_valu_cases.py), the smallest size at which a radius-5 ring still has full and border-cut rings and
the block region has more than one 16 x 16 block per side.

run_case(name, fit_side) -> {array name: array}; fit_side None leaves the option alone (a library from before it existed).  `info` rows are
(first_run, frame_stride, n_active, pmax) of each fit; W is kept as the bits of NROWS sampled pixel rows, b0 as every third pixel."""
import numpy as np

D, T, K, SEED = 48, 300, 8, 17
NROWS, ROW_SEED = 32, 20261

# ---- full iterations (background, spatial, temporal) through Sources2D: name -> settings ----
SRC = {
    # (i) radius 5, three iterations: the first fit builds the video's table, the second is the first steady-state fit, the third runs after the spatial and the
    #     temporal update have been through the shared scratch
    "i_r5": dict(iters=3, profile=True),
    # (ii) the fp32 window projection
    "ii_fp32": dict(iters=3, profile=True, opts={"win_i8": 0}),
    # (iii) the table path: k_cov_correct reads the pair list and the need masks in EVERY fit
    "iii_table": dict(opts={"solve_packed": 0}),
    # (iv) the outlier branch: the direct Gram of a clipped Bf, every table in every fit
    "iv_outlier": dict(okw={"thresh_outlier": 5.0}),
    # (vii) the low-resolution fit of bg_ssub = 2
    "vii_ssub2": dict(okw={"bg_ssub": 2}),
    # (viii) 2 x 2 patches, on one lane and on two
    "viii_lanes1": dict(dims=(96, 96), pdims=[48, 48], nrows=16),
    "viii_lanes2": dict(dims=(96, 96), pdims=[48, 48], nrows=16, lanes=2),
    # (x) the CSR-walking packed solve: no staged windows, so no metadata upload
    "x_unstaged": dict(opts={"solve_staged": 0}),
}
DIRECT = ("v_stride", "vi_empty", "ix_two_engines")
CASES = tuple(SRC) + DIRECT
STRIDE_T, STRIDE_R, STRIDE_M = 1500, 2, (None, 6, 6, 16, 6)     # (v): positive weights per row set before each fit -> 100 pmax = 600, 600, 1600, 600 against T = 1500
STRIDES = (1, 2, 2, 1, 2)


def sample_rows(d, n=NROWS):
    return np.sort(np.random.default_rng(ROW_SEED).choice(d, size=n, replace=False))


def _bits(x):
    return np.ascontiguousarray(x, dtype=np.float32).view(np.uint32)


def _info(i):
    return np.array([int(i["first_run"]), i["frame_stride"], i["n_active"], i["pmax"]], dtype=np.int64)


def _engine(fit_side, opts=None, lanes=1):
    from cnmf_e_amd.engine import Engine
    eng = Engine(0)
    if lanes > 1:
        eng.set_option("lanes", lanes)
    if fit_side is not None:
        eng.set_option("fit_side", fit_side)
    for k, v in (opts or {}).items():
        eng.set_option(k, v)
    return eng


def _kept(out, tag, eng, pid, info, rows):
    W = eng.ring_csr(pid)
    out[tag + "_W"] = _bits(W[rows].data)
    out[tag + "_b0"] = _bits(eng.b0(pid)[::3])
    out[tag + "_info"] = _info(info)
    assert np.all(np.isfinite(W.data))
    return W


def run_src(fit_side, dims=(D, D), pdims=None, r=5, iters=2, opts=None, okw=None, lanes=1, profile=False, nrows=NROWS):
    from cnmf_e_amd import synth
    from cnmf_e_amd.sources2d import PatchedVideo, Sources2D, Options
    f = synth.make_factors(dims[0], dims[1], T, K, SEED, gSig=2.0, gSiz=9, min_sep=5)
    Y = synth.make_video(f, np.float32)
    eng = _engine(fit_side, opts, lanes)
    out, kernels = {}, []
    try:
        video = PatchedVideo(dims[0], dims[1], T, pdims or list(dims), r, eng)
        video.upload_from_full(Y)
        kw = dict(spatial_algorithm="hals", maxIter=3); kw.update(okw or {})
        s = Sources2D(video, Options(ring_radius=r, **kw), f.A_init, f.C_init, f.sn)
        if profile:
            eng.profile(True)
        for it in range(iters):
            if profile:
                eng.profile_reset()
            infos = s.update_background_parallel()
            if profile:
                kernels.append({n for n, v in eng.profile_table().items() if v["calls"] > 0})
            for n, idx in enumerate(video.owned):
                if idx in infos:
                    W = s.get_W(idx)                              # (bg_ssub > 1: of the low-resolution patch)
                    rows = sample_rows(W.shape[0], nrows)
                    out["it%d_p%d_W" % (it, n)] = _bits(W[rows].data)
                    out["it%d_p%d_b0" % (it, n)] = _bits(eng.b0(video.pid[idx])[::3])
                    out["it%d_p%d_info" % (it, n)] = _info(infos[idx])
            s.update_spatial_parallel()
            s.update_temporal_parallel()
        A = s.A.tocsc(); A.sort_indices()
        out["A_indptr"], out["A_indices"], out["A_data"] = A.indptr.astype(np.int32), A.indices.astype(np.int32), _bits(A.data)
        out["C"] = _bits(np.asarray(s.C, dtype=np.float32))
        eng.synchronize()
    finally:
        eng.close()
    return out, kernels


def _direct_inputs(t=T):
    from cnmf_e_amd import synth
    f = synth.make_factors(D, D, t, K, SEED, gSig=2.0, gSiz=9, min_sep=5)
    return f, synth.make_video(f, np.float32)


def _patch(eng, Y, t, r):
    from cnmf_e_amd.sources2d import PatchedVideo
    video = PatchedVideo(D, D, t, [D, D], r, eng)
    video.upload_from_full(Y)
    eng.ring_init(0, r)
    return video


def set_positive(W, m):
    """values for ring_set_values: per pixel row the first m stored weights positive, the rest negative, all distinct (so pmax = m, and no first run)"""
    val = np.empty(W.nnz, dtype=np.float32)
    for i in range(W.shape[0]):
        lo, hi = W.indptr[i], W.indptr[i + 1]
        j = np.arange(hi - lo)
        val[lo:hi] = np.where(j < m, 0.01, -0.01) * (j + 1)
    return val


def run_stride(fit_side):
    """(v) radius 2 (16 ring pixels), T = 1500: the number of positive weights per row is SET before each fit, so the stride T // min(T, 100 pmax) goes 1, 2, 2, 1, 2.
    Fit 2 builds the second table, fit 3 is a steady-state fit on the fp32 strided projection, fit 4 swaps the first table back in (its trace digits are only
    queued once the stride is known), fit 5 swaps again.  -> (arrays, [the W each fit started from])"""
    f, Y = _direct_inputs(STRIDE_T)
    fits = [(f.A_init, f.C_init), (f.A_true, f.C_true), (f.A_init, f.C_init), (f.A_true, f.C_true), (f.A_init, f.C_init)]
    eng = _engine(fit_side)
    out, before = {}, []
    try:
        _patch(eng, Y, STRIDE_T, STRIDE_R)
        rows = sample_rows(D * D)
        for k, ((A, C), m) in enumerate(zip(fits, STRIDE_M)):
            W = eng.ring_csr(0)
            if m is not None:
                W = W.copy(); W.data = set_positive(W, m)
                eng.ring_set_values(0, W.data)
            before.append(W)
            _, info = eng.fit_ring_model(0, A.tocsc().astype(np.float32), np.ascontiguousarray(C, dtype=np.float32))
            _kept(out, "fit%d" % k, eng, 0, info, rows)
    finally:
        eng.close()
    return out, before


def run_empty(fit_side):
    """(vi) no neuron at all (A = [], K = 0), then an A whose fourth column is empty, twice"""
    import scipy.sparse as sp
    f, Y = _direct_inputs()
    A = f.A_true.tolil(copy=True); A[:, 3] = 0
    A = sp.csc_matrix(A).astype(np.float32); A.eliminate_zeros()
    assert A.indptr[3] == A.indptr[4] and A.nnz > 0
    C = np.ascontiguousarray(f.C_true, dtype=np.float32)
    fits = [(f.A_init.tocsc().astype(np.float32), np.ascontiguousarray(f.C_init, dtype=np.float32)), (None, None), (A, C), (A, C)]
    eng = _engine(fit_side)
    out = {}
    try:
        _patch(eng, Y, T, 5)
        rows = sample_rows(D * D)
        for k, (Ak, Ck) in enumerate(fits):
            _, info = eng.fit_ring_model(0, Ak, Ck)
            _kept(out, "fit%d" % k, eng, 0, info, rows)
    finally:
        eng.close()
    return out


def run_two_engines(fit_side):
    """(ix) two engines alive at once, each with its own side stream, fitting alternately (the second at another radius)"""
    f, Y = _direct_inputs()
    fits = [(f.A_init, f.C_init), (f.A_true, f.C_true), (f.A_init, f.C_init)]
    engs = [_engine(fit_side), _engine(fit_side)]
    out = {}
    try:
        for e, r in zip(engs, (5, 8)):
            _patch(e, Y, T, r)
        rows = sample_rows(D * D)
        for k, (A, C) in enumerate(fits):
            for n, e in enumerate(engs):
                _, info = e.fit_ring_model(0, A.tocsc().astype(np.float32), np.ascontiguousarray(C, dtype=np.float32))
                _kept(out, "e%d_fit%d" % (n, k), e, 0, info, rows)
    finally:
        for e in engs:
            e.close()
    return out


def run_case(name, fit_side):
    """-> (arrays, extra): extra = the kernel names per background update (profiled Sources2D cases), the starting weights per fit (v), else None"""
    if name in SRC:
        return run_src(fit_side, **SRC[name])
    if name == "v_stride":
        return run_stride(fit_side)
    if name == "vi_empty":
        return run_empty(fit_side), None
    if name == "ix_two_engines":
        return run_two_engines(fit_side), None
    raise KeyError(name)
