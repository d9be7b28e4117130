"""The runs of tests/test_gpu_residual_state.py and of scripts/make_residual_state_golden.py (which recorded tests/golden/residual_state_parent.npz with them, on the
parent commit's library): scripted engine-level sequences that take the residual of a patch through every transition of its state ("Residual state") --
fit, record, pend, fold, realise, export, invalidate, sweep -- under every option that changes the plan.  Shapes are the smallest at which each path exists, taken
from tests/test_gpu_virtual.py (44 x 40, radius 5: the LDS-DMA small ring; 64 x 64, radius 15: the duo kernel and the deferred term exist only there) and
tests/test_gpu_ssub_virtual.py (96 x 80, radius 10, bg_ssub = 2).

run_case(name) -> {array name: array} on a fresh engine.  Arrays of up to FULL elements are kept whole (as bits), larger ones as SAMPLE fixed entries plus two
checksums of the WHOLE array (the wrapping uint64 sum of its uint32 view, plain and weighted by position): the file has to stay small, and a single changed bit
anywhere still changes both sums.  The two exports are kept as 64 fixed pixels x 16 fixed frames + the sums.  `kernels` / `calls` are the profile table's call
counts of the residual's kernels (PREFIXES) over the whole sequence."""
import numpy as np

PREFIXES = ("residual_", "r1_", "ssub_", "ysig_", "spatial_term", "temporal_term", "spatial_from_ptab", "spatial_proj", "spatial_ptab", "temporal_proj")
FULL, SAMPLE, SEED = 1024, 256, 20271
NOT_RUN = "cnmfe_residual has not been run for patch 0"
RSS_SSUB = "compute_RSS needs the residual of cnmfe_residual (bg_ssub = 1)"

SHAPES = {"r5": dict(dims=(44, 40), T=96, r=5, K=6), "r15": dict(dims=(64, 64), T=160, r=15, K=6), "ssub": dict(dims=(96, 80), T=400, r=10, K=12, ssub=2)}
OPTS = {"default": {}, "virtual0": {"r1_virtual": 0}, "lazy0": {"r1_lazy": 0}, "delta0": {"r1_delta": 0}, "defer0": {"r1_defer": 0}}
CASES = {}
for _s in ("r5", "r15"):
    for _o, _v in OPTS.items():
        CASES["%s_%s" % (_s, _o)] = (_s, _v)
for _v in (-1, 10, 11):
    CASES["r15_variant%d" % _v] = ("r15", {"r1_variant": _v})
CASES["ssub_sweep"] = ("ssub", {"ssub_virtual": 0})
CASES["ssub_virtual"] = ("ssub", {"ssub_virtual": 2})
CASES["ssub_virtual_lazy0"] = ("ssub", {"ssub_virtual": 2, "r1_lazy": 0})


def _sums(x):
    u = np.ascontiguousarray(x).view(np.uint32).ravel().astype(np.uint64)
    w = (np.arange(u.size, dtype=np.uint64) % np.uint64(65521)) + np.uint64(1)
    return np.array([u.sum(dtype=np.uint64), (u * w).sum(dtype=np.uint64)], dtype=np.uint64)


def record(out, name, x):
    x = np.ascontiguousarray(x)
    if x.dtype == np.float64:
        x = x.view(np.uint64).view(np.uint32)
    elif x.dtype == np.float32:
        x = x.view(np.uint32)
    if x.size <= FULL:
        out[name] = x
        return
    idx = np.sort(np.random.default_rng(SEED).choice(x.size, size=SAMPLE, replace=False))
    out[name + "_sample"] = x.ravel()[idx]
    out[name + "_sums"] = _sums(x)


def record_export(out, name, y):
    """y: (T, d) float32"""
    rng = np.random.default_rng(SEED)
    px, fr = np.sort(rng.choice(y.shape[1], size=64, replace=False)), np.sort(rng.choice(y.shape[0], size=16, replace=False))
    out[name + "_rows"] = np.ascontiguousarray(y[np.ix_(fr, px)]).view(np.uint32)
    out[name + "_sums"] = _sums(y)


def _raises(fn, message):
    from cnmf_e_amd._lib import CnmfeError
    try:
        fn()
    except CnmfeError as e:
        assert message in str(e), str(e)
        return np.array(str(e).split(": ", 1)[1])
    raise AssertionError("no error: " + message)


def run_case(name):
    import scipy.sparse as sp
    from scipy.ndimage import binary_dilation
    from cnmf_e_amd import synth
    from cnmf_e_amd.engine import Engine
    from cnmf_e_amd.sources2d import PatchedVideo
    shape, opts = CASES[name]
    g = SHAPES[shape]
    (d1, d2), T, r, K, ssub = g["dims"], g["T"], g["r"], g["K"], g.get("ssub", 1)
    f = synth.make_factors(d1, d2, T, K, 31, gSig=1.5, gSiz=7, min_sep=5)
    Y = synth.make_video(f, np.float32)
    A = f.A_init.tocsc().astype(np.float32)
    Cm = np.ascontiguousarray(f.C_init, dtype=np.float32)
    img = (A.toarray() > 0).reshape(d1, d2, -1, order="F")
    IND = sp.csc_matrix(np.stack([binary_dilation(img[:, :, k], structure=np.ones((3, 3), bool)) for k in range(K)], axis=2).reshape(d1 * d2, -1, order="F")).astype(np.float32)
    prev = np.array([0, 3, 4])
    out = {}
    eng = Engine(0)
    try:
        for k, v in opts.items():
            eng.set_option(k, v)
        video = PatchedVideo(d1, d2, T, [d1, d2], r, eng)
        video.upload_from_full(Y)
        eng.ring_init(0, r)
        if ssub > 1:
            rr = -(-r // ssub)
            eng.patch_derive(0, 1, ssub, "nearest"); eng.patch_derive(0, 2, ssub, "bicubic")
            eng.ring_init(1, rr); eng.ring_init(2, rr)
            fit = lambda: eng.fit_ring_model_ssub(0, 1, 2, ssub, A, Cm)
            residual = lambda *a, **kw: eng.residual_ssub(0, 2, ssub, *a, **kw)
        else:
            fit = lambda: eng.fit_ring_model(0, A, Cm)
            residual = lambda *a, **kw: eng.residual(0, *a, **kw)
        eng.profile(True); eng.profile_reset()
        fit()                                                            # 1
        b0 = eng.b0(0)
        record(out, "01_b0", b0)
        residual()                                                       # 2: no footprints
        residual(A[:, prev], Cm[prev])                                   # 3: a term pends
        Anew = eng.update_spatial(0, "hals", A, Cm, IND).tocsc()         # 4
        Anew.sort_indices()
        record(out, "04_A_indptr", Anew.indptr.astype(np.int32)); record(out, "04_A_indices", Anew.indices.astype(np.int32)); record(out, "04_A_data", Anew.data.astype(np.float32))
        residual(A, Cm)                                                  # 5
        for n, x in zip(("C", "Craw", "aa"), eng.hals_temporal(0, Anew, Cm, 3)):     # 6
            record(out, "06_" + n, x)
        record(out, "07_sn", eng.get_sn(0))                              # 7: realises and folds
        record_export(out, "08_ysig", residual(want=True))               # 8: an export
        if ssub > 1:
            out["09_rss_error"] = _raises(lambda: eng.compute_rss(0, A, Cm, b0, b0), RSS_SSUB)
            eng.set_b0(0, b0)                                            # invalidates
            record_export(out, "10_ysig", residual(A, Cm, want=True))
        else:
            eng.ring_set_values(0, eng.ring_csr(0).data)                 # 9: the same values; invalidates
            record_export(out, "10_ysig", residual(A, Cm, want=True))    # 10
            record(out, "11_rss", np.array([eng.compute_rss(0, A, Cm, b0, b0)]))              # 11
            record(out, "12_bg", eng.reconstruct_background(0, b0, b0, 0, 8))                # 12
        eng.set_b0(0, b0)                                                # 13: invalidates again
        out["14_error"] = _raises(lambda: eng.fast_temporal(0, A), NOT_RUN)                   # 14
        eng.synchronize()
        tab = {k: v["calls"] for k, v in eng.profile_table().items() if v["calls"] > 0 and k.startswith(PREFIXES)}
        out["kernels"] = np.array(sorted(tab))
        out["calls"] = np.array([tab[k] for k in sorted(tab)], dtype=np.int64)
    finally:
        eng.close()
    return out
