"""TEST INFRASTRUCTURE of the long-recording tests (tests/test_gpu_long_*.py, tests/test_long_fixtures.py): the runners that repeat an existing fixture under
option trace_long, and the fixtures at the three long frame counts

    20 417   the first count the LDS flavours cannot take: n % 4 = 1, odd median, nfft = 8192, the transform's tables in LDS
    40 001   nfft = 16384, the tables in global memory
    74 000   even median, nfft = 32768, the split transform

with their float64 oracles, computed once per process and left read-only."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, os.path.join(ROOT, "oracle"))
sys.path.insert(0, HERE)

import oasis_oracle as oo
import seed_oracle as so
import greedy_oracle as go
import greedy_cases as gc
from cnmf_e_amd import synth

T_LONG = (20417, 40001, 74000)
SN_TOL = 2e-4         # relative: what tests/test_gpu_edges.py::test_get_sn_of_long_recordings asserts of the same Welch estimator at these lengths
_cache = {}


def _once(key, fn):
    if key not in _cache:
        _cache[key] = fn()
    return _cache[key]


class _Geometry:
    def create_patch(self, *a):
        pass


def engine(trace_long=None):
    """a fresh Engine; trace_long None: the option is never set"""
    from cnmf_e_amd.engine import Engine
    eng = Engine(0)
    if trace_long is not None:
        eng.set_option("trace_long", trace_long)
    return eng


# ---- the existing fixtures under option trace_long (test_gpu_long_flavour.py) --------------------------------------------------------------------------------
def seed_images_run(case, trace_long):
    """correlation_pnr_parallel of a case of tests/test_gpu_seed_images.py -> (Cn, PNR, {patch: the peel open's (Cn, PNR, Sn) of its block})"""
    from cnmf_e_amd.sources2d import PatchedVideo, Sources2D, Options
    c = dict(case)
    d1, d2 = c["dims"]
    f = synth.make_factors(d1, d2, c["T"], c["K"], c["seed"], gSig=c["gSig"], gSiz=int(c.get("synth_gSiz", c["gSiz"])))
    Y = synth.make_video(f, np.float32)
    eng = engine(trace_long)
    try:
        video = PatchedVideo(d1, d2, c["T"], c["pdims"] or [d1, d2], c["r"], eng)
        video.upload_from_full(Y)
        s = Sources2D(video, Options(ring_radius=c["r"], gSig=c["gSig"], gSiz=c["gSiz"], center_psf=c.get("center_psf", True), nk=c.get("nk", 1)), f.A_init, f.C_init, f.sn)
        Cn, PNR = s.correlation_pnr_parallel(c.get("frame_range"))
        # Sn, which the method does not return: the peel session's open of every patch with the method's own arguments (its Cn / PNR are the same kernels' output)
        from cnmf_e_amd.sources2d import seed_psf, bspline_basis
        fr = c.get("frame_range")
        n = c["T"] if fr is None else fr[1]
        nk = c.get("nk", 1)
        psf = seed_psf(float(c["gSig"]), float(c["gSiz"]), bool(c.get("center_psf", True)))
        Q = np.linalg.qr(bspline_basis(n, nk))[0] if nk > 1 else None
        Sn = {}
        for idx in video.owned:
            Sn[idx] = eng.peel_open(video.pid[idx], psf, n, Q, 3.0)
            eng.peel_close(video.pid[idx])
        return Cn, PNR, Sn
    finally:
        eng.close()


def greedy_run(name, trace_long):
    """initComponents_parallel of a case of tests/greedy_cases.py under the oracle's accepted centres as forced seeds, with the step observer"""
    from cnmf_e_amd.sources2d import PatchedVideo, Sources2D
    c = gc.CASES[name]
    f, Y = gc.inputs(name)
    d1, d2 = c["dims"]
    eng = engine(trace_long)
    try:
        video = PatchedVideo(d1, d2, c["T"], c["pdims"] or [d1, d2], c["r"], eng)
        video.upload_from_full(Y)
        s = Sources2D(video, gc.options(name), f.A_init, f.C_init, f.sn)
        log = {}
        s._init_observer = lambda idx, kind, data: log.setdefault(idx, []).append((kind, data))
        seeds = [tuple(int(x) for x in rc) for rc in gc.oracle(name)["center"]]
        center, Cn, PNR = s.initComponents_parallel(K=c.get("Kmax"), frame_range=c.get("frame_range"), seeds=seeds)
        return dict(center=center, Cn=Cn, PNR=PNR, A=s.A.toarray(), C=np.array(s.C), C_raw=np.array(s.C_raw), S=np.array(s.S), steps=log)
    finally:
        eng.close()


def residual_run(name, trace_long):
    """initComponents_residual_parallel (automatic search) of a case of tests/residual_cases.py, with the observer"""
    import residual_cases as rc
    from cnmf_e_amd.sources2d import PatchedVideo, Sources2D
    c = rc.CASES[name]
    f, Y, A0, C0 = rc.inputs(name)
    d1, d2 = c["dims"]
    eng = engine(trace_long)
    try:
        video = PatchedVideo(d1, d2, c["T"], rc.pdims(c), c["r"], eng)
        video.upload_from_full(Y)
        s = Sources2D(video, rc.options(name), A0, C0, f.sn)
        s.update_background_parallel()
        K_old = s.A.shape[1]
        s.ids = np.arange(11, 11 + K_old); s.tags = np.zeros(K_old, dtype=np.uint16); s.P["k_ids"] = 10 + K_old
        log = {}
        s._init_observer = lambda idx, kind, data: log.setdefault(idx, []).append((kind, data))
        center, Cn, PNR = s.initComponents_residual_parallel(min_corr=c["min_corr"], min_pnr=c["min_pnr"])
        return dict(center=center, Cn=Cn, PNR=PNR, A=s.A.toarray(), C=np.array(s.C), C_raw=np.array(s.C_raw), steps=log)
    finally:
        eng.close()


def equal_tree(a, b):
    """np.array_equal (NaNs in the same places) over nested dicts / lists / tuples of arrays and scalars; returns the path of the first difference or None"""
    if isinstance(a, dict):
        if set(a) != set(b):
            return "keys"
        for k in a:
            r = equal_tree(a[k], b[k])
            if r is not None:
                return "%s.%s" % (k, r)
        return None
    if isinstance(a, (list, tuple)):
        if len(a) != len(b):
            return "len"
        for i, (x, y) in enumerate(zip(a, b)):
            r = equal_tree(x, y)
            if r is not None:
                return "%d.%s" % (i, r)
        return None
    if a is None or b is None:
        return None if a is b else "none"
    x, y = np.asarray(a), np.asarray(b)
    if x.shape != y.shape:
        return "shape"
    if x.dtype.kind in "fc":
        return None if np.array_equal(x, y, equal_nan=True) else "values"
    return None if np.array_equal(x, y) else "values"


# ---- long traces for the merge / tag calls (test_gpu_long_merge.py) --------------------------------------------------------------------------------------------
def traces_long(T, K=5):
    """(C, C_raw, S) K x T float32, built like merge_cases.traces / merge_cases.case: AR(1) transients plus noise as C_raw, the noiseless trace as C, its
    innovations as S; row 1 is nearly row 0"""
    def make():
        rng = np.random.default_rng(7 + T)
        S = (rng.random((K, T)) < 0.02) * rng.uniform(5.0, 15.0, (K, T))
        C = np.stack([synth._ar1(s, 0.95) for s in S])
        C[1] = C[0] + 0.05 * rng.normal(0.0, 1.0, T)
        R = C + rng.normal(0.0, 0.3, (K, T)) + 0.7
        out = tuple(np.ascontiguousarray(a, dtype=np.float32) for a in (C, R, S))
        for a in out:
            a.setflags(write=False)
        return out
    return _once(("traces", T, K), make)


DIFF_MARGIN = 1.2e-3  # |d - 2 sn| / sn below which a sample of the difference trace is left out: 2 x SN_TOL x 3
DIFF_LEFT_MAX = 1e-3  # at most this share of a trace's samples


def diff_oracle(T, K=5):
    """(sn (K), S_ (K x T), margin (K x T)) of merge_high_corr.m:57-66 in float64 on the fp32 values"""
    def make():
        R = traces_long(T, K)[1].astype(np.float64)
        D = np.c_[np.diff(R, axis=1), np.zeros(K)]
        sn = np.array([oo.GetSn(d) for d in D])
        out = (sn, np.where(D < 2.0 * sn[:, None], 0.0, D), np.abs(D - 2.0 * sn[:, None]) / sn[:, None])
        for a in out:
            a.setflags(write=False)
        return out
    return _once(("diff", T, K), make)


MERGE_T = 40001
MERGE_DIMS = (12, 10)
MERGE_THR = [0.1, 0.5, 0.3]
MERGE_MIN_PIXEL = 5


def merge_case():
    """the situations of merge_cases.case that the long path must tell apart, on a 12 x 10 field of view and 40 001 frames.  Seven neurons:
        0, 6   the two halves of a split neuron (three pixel columns shared), traces 0.6 x0 and x0 + small noise   -> {0, 6} merge
        1      an ordinary neuron, 2 a silent one (S = 0: tag 2), 3 with C_raw == C (tag 4), 4 three pixels (tag 1), 5 an ordinary neuron close to 1, uncorrelated
    C, S, kernel_pars: the float64 oracle's deconvTemporal of the raw traces, stored as float32.  dict as merge_cases.case."""
    def make():
        import scipy.sparse as sp
        d1, d2 = MERGE_DIMS
        T = MERGE_T
        rng = np.random.default_rng(4001)
        rr, cc = np.meshgrid(np.arange(d1), np.arange(d2), indexing="ij")
        def blob(r, c, s=1.5):
            g = np.exp(-((rr - r) ** 2 + (cc - c) ** 2) / (2 * s * s)); g[g < 0.05] = 0
            return g
        ar = lambda: synth._ar1((rng.random(T) < 0.02) * rng.uniform(5.0, 15.0, T), 0.95)
        noise = lambda s=0.3: rng.normal(0.0, s, T)
        x = [ar() for _ in range(5)]
        A = np.zeros((d1 * d2, 7)); R = np.zeros((7, T))
        img = blob(3, 4)
        left, right = img.copy(), img.copy()
        left[:, 6:] = 0; right[:, :3] = 0
        A[:, 0] = left.ravel(order="F"); A[:, 6] = right.ravel(order="F")
        R[0] = 0.6 * (x[0] + noise(0.1)); R[6] = x[0] + noise(0.1)
        A[:, 1] = blob(9, 2).ravel(order="F"); R[1] = x[1] + noise()
        A[:, 2] = blob(9, 7).ravel(order="F"); R[2] = x[2] + noise()
        A[:, 3] = blob(6, 8).ravel(order="F"); R[3] = x[3] + noise()
        A[[0, 1, 2], 4] = [1.0, 0.8, 0.6]; R[4] = x[4] + noise()
        A[:, 5] = blob(9, 4).ravel(order="F"); R[5] = ar() + noise()
        R += 0.7
        R32 = R.astype(np.float32)
        Cd, Rd, Sd, kp, _ = oo.deconvTemporal(R32.astype(np.float64))
        C = Cd.astype(np.float32); Craw = Rd.astype(np.float32); S = Sd.astype(np.float32); kp = np.asarray(kp, dtype=np.float32)
        S[2] = 0.0
        Craw[3] = C[3]
        A32 = A.astype(np.float32)
        Y = (Craw.T.astype(np.float64) @ A32.T.astype(np.float64) + 100.0 + rng.normal(0.0, 1.0, (T, d1 * d2))).astype(np.float32)
        for v in (C, Craw, S, kp, Y):
            v.setflags(write=False)
        return dict(d1=d1, d2=d2, T=T, A=sp.csc_matrix(A32), C=C, C_raw=Craw, S=S, kernel_pars=kp, video=Y, sn=np.ones(d1 * d2, dtype=np.float32))
    return _once(("merge_case",), make)


def merge_oracle_runs():
    """(merge_high_corr's result, (tags, tag margins), (ids, kept arrays) of remove_false_positives) of tests/merge_oracle.py on merge_case()"""
    def make():
        import merge_oracle as mo
        c = merge_case()
        args = (c["A"], c["C"], c["C_raw"], c["S"], c["kernel_pars"])
        return (mo.merge_high_corr(*args, MERGE_THR), mo.tag_neurons(*args[:4], MERGE_MIN_PIXEL), mo.remove_false_positives(*args, MERGE_MIN_PIXEL))
    return _once(("merge_oracle",), make)


# ---- the peel session at long T (test_gpu_long_init.py) -------------------------------------------------------------------------------------------------------
# 30 x 28 pixels, K = 2 true neurons, gSig 2, gSiz 9, nk = 1, one patch, the demo's min_corr 0.8 / min_pnr 8.  The events of the two neurons are five times the
# synthesiser's (amp): at its own amplitude the slowly varying background field, whose Gaussians are neuron-sized in so small a field of view and which nk = 1
# leaves in, leads the search and the neurons' traces come out as the mean of a few noisy pixels.  The synthetic seed of each count was found by scanning seeds
# 0, 1, 2, ... on the CPU until the corr margins of the oracle's automatic search and of its forced run cleared greedy_cases.MARGIN_MIN["corr"]; at 20 417 frames
# (the end-to-end call) also until a centre lay within 2 pixels of each true one and its C row correlated above 0.9 with the true trace (seed 2: 0.994 and 0.989;
# the search accepts five centres there, the two neurons and three blobs of the background).  At 74 000 frames the search is capped at two neurons (PEEL_KMAX), which
# keeps the oracle's run short.  PEEL_CENTRES: the accepted centres of the automatic search (1-based), which tests/test_long_fixtures.py pins.
PEEL = dict(dims=(30, 28), K=2, gSig=2.0, gSiz=9, r=6, min_corr=0.8, min_pnr=8.0, noise_sd=1.0, amp=5.0)
PEEL_KMAX = {20417: None, 74000: 2}
PEEL_SEED = {20417: 2, 74000: 2}
PEEL_CENTRES = {20417: [(6, 18), (22, 8), (11, 11), (20, 20), (10, 5)], 74000: [(8, 17), (25, 22)]}


def peel_video(T):
    def make():
        d1, d2 = PEEL["dims"]
        import dataclasses
        f = synth.make_factors(d1, d2, T, PEEL["K"], PEEL_SEED[T], gSig=PEEL["gSig"], gSiz=PEEL["gSiz"], noise_sd=PEEL["noise_sd"])
        f = dataclasses.replace(f, C_true=(PEEL["amp"] * f.C_true).astype(np.float32))          # larger events: the neurons, not the slow background, lead the search
        Y = synth.make_video(f, np.float32)
        Y.setflags(write=False)
        return f, Y
    return _once(("peel_video", T), make)


def peel_geometry(T):
    from cnmf_e_amd.sources2d import PatchedVideo
    d1, d2 = PEEL["dims"]
    return PatchedVideo(d1, d2, T, [d1, d2], PEEL["r"], _Geometry())


def peel_oracle(T, forced=True):
    """greedy_oracle.greedy_fov of the fixture: the automatic search, or (forced) the run under PEEL_CENTRES[T] as seeds.  The forced run's extract steps also
    carry what cnmfe_peel_extract reports beside corr, ci, ai: norm_ci, sn_ci = GetSn(ci), max_diff / std_diff of diff(y0), y0 the centre's HY trace at that step
    (rebuilt from the run's own results: HY0(p) - sum_j Hai_j(p) ci_j over the neurons applied before)."""
    def make():
        _, Y = peel_video(T)
        seeds = [tuple(int(x) for x in rc) for rc in PEEL_CENTRES[T]] if forced else None
        res = go.greedy_fov(Y, peel_geometry(T), PEEL["gSig"], PEEL["gSiz"], seeds=seeds, min_corr=PEEL["min_corr"], min_pnr=PEEL["min_pnr"], K=PEEL_KMAX[T])
        if forced:
            d1, d2 = PEEL["dims"]
            psf = so.make_psf(PEEL["gSig"], PEEL["gSiz"], True)
            blk = res["blocks"][(0, 0)]
            done = 0
            for st in blk["steps"]:
                if st["kind"] == "apply":
                    done += 1
                    continue
                r, c = st["r"], st["c"]
                R = so.matlab_round(PEEL["gSiz"])
                r0, r1, c0, c1 = max(0, r - R), min(d1, r + R + 1), max(0, c - R), min(d2, c + R + 1)
                win = Y[:, [cc * d1 + rr for cc in range(c0, c1) for rr in range(r0, r1)]].astype(np.float64).T.reshape(r1 - r0, c1 - c0, -1, order="F")
                # the filter reaches 4 pixels: the 19 x 19 window around the centre holds everything its filtered trace reads (replicate padding only at the image edge)
                y0 = so.imfilter_replicate(win, psf)[r - r0, c - c0]
                y0 = y0 - np.median(y0)
                for j in range(done):
                    (a0, a1, b0, b1), ai = blk["A"][j]
                    s0, s1, t0, t1 = go._box(d1, d2, int(blk["center"][j, 0]) - 1, int(blk["center"][j, 1]) - 1, 2 * PEEL["gSiz"])
                    big = np.zeros((s1 - s0, t1 - t0)); big[a0 - s0:a1 - s0, b0 - t0:b1 - t0] = ai
                    Hai = so.imfilter_replicate(big[:, :, None], psf)[:, :, 0]        # (filtered inside the updated box, as greedyROI_endoscope.m:385 does)
                    if s0 <= r < s1 and t0 <= c < t1:
                        y0 = y0 - Hai[r - s0, c - t0] * blk["C_raw"][j]
                dy = np.diff(y0)
                st["stats"] = dict(norm_ci=float(np.linalg.norm(st["ci"])), sn_ci=float(oo.GetSn(st["ci"])), max_diff=float(dy.max()), std_diff=float(dy.std(ddof=1)))
        return res
    return _once(("peel_oracle", T, forced), make)


# ---- seed images at long T (test_gpu_long_seed.py) ----------------------------------------------------------------------------------------------------------
SEED = dict(dims=(20, 18), K=2, seed=5, gSig=1.5, gSiz=7, r=3, nk=3)      # one patch: tiles of 16 + 4 rows and 16 + 2 columns
SEED_DELTA = 2e-3     # the quantised video: a pixel is fragile when the oracle's margin is below sig = 3 times the 2e-4 relative Sn bound, times 3, rounded up
SEED_LEFT_MAX = 0.10


def seed_video(T):
    def make():
        d1, d2 = SEED["dims"]
        f = synth.make_factors(d1, d2, T, SEED["K"], SEED["seed"], gSig=SEED["gSig"], gSiz=SEED["gSiz"])
        Y = synth.make_video(f, np.float32)
        Y.setflags(write=False)
        return f, Y
    return _once(("seed_video", T), make)


def seed_video_q(T):
    """Y4 = 4 rint(Y / 4) as float32: multiples of 4 are exact, HY - median sits on a grid of spacing 4 that the threshold rarely meets"""
    def make():
        Y4 = (4.0 * np.rint(seed_video(T)[1].astype(np.float64) / 4.0)).astype(np.float32)
        Y4.setflags(write=False)
        return Y4
    return _once(("seed_video_q", T), make)


def seed_oracle_q(T):
    """(Cn, PNR, robust) of the quantised video with no filter and no detrend, d1 x d2 images; robust: neither the pixel nor a neighbour is fragile"""
    def make():
        d1, d2 = SEED["dims"]
        cn, pnr, margin = so.seed_images(seed_video_q(T).T.astype(np.float64), d1, d2, 0.0, 0, True, 1, 3.0)
        out = (cn, pnr, ~so.dilate8(margin < SEED_DELTA))
        for a in out:
            a.setflags(write=False)
        return out
    return _once(("seed_oracle_q", T), make)


def seed_oracle_pnr(T):
    """PNR (d1 x d2) of the filtered (gSig 1.5, center_psf), detrended (nk = 3) float video"""
    def make():
        d1, d2 = SEED["dims"]
        _, pnr, _ = so.filtered_traces(seed_video(T)[1].T.astype(np.float64), d1, d2, SEED["gSig"], SEED["gSiz"], True, SEED["nk"], 3.0)
        pnr = pnr.reshape(d1, d2, order="F")
        pnr.setflags(write=False)
        return pnr
    return _once(("seed_oracle_pnr", T), make)
