"""Where extract_DF_F_endoscope spends its time at the headline size: 512 x 512 x 10000, K = 500, as one patch (--config c3) or as the 4 x 4 patches of
BASELINE configs[3] (--config c4), after one background + spatial + temporal iteration.

  whole call            wall time of extract_DF_F_endoscope() between two device fences, for (df_prctile, df_window) = (50, None) and (20, 1000): the first call of
                        the session on its own, then the median of three with the profiler off
  phases                the engine's per-kernel HIP events (Engine.profile: one event pair around every launch), in a run of their own: reconstruction of the
                        chunks (rss_const + bg_reconstruct), df_project, df_scale, df_base / df_base_win, df_divide, and whatever else the call launched
                        (the residual's realisation, uploads)
  df_project's traffic  sum_k nnz_k * T * 4 bytes (the gathered background samples) against its summed kernel time
  --host-route          for comparison the only route the parent commit offers: reconstruct_background() to the host (d1 x d2 x T float32) and the same sparse
                        product in SciPy, then the float64 oracle's median -- same code on this commit, the method is unchanged

One JSON line per measurement on stdout.  python scripts/df_probe.py --config c3 [--host-route] [--window 16384]"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def baseline_only(a):
    """the baseline kernels without a video: a window of 16384 frames needs a recording at least that long (a longer window means none, Sources2D.m:546)"""
    import torch
    from cnmf_e_amd.engine import Engine
    K, T = 500, a.baseline_T
    rng = np.random.default_rng(0)
    Yf = np.cumsum(rng.standard_normal((K, T)), axis=1) + 500
    Cm = rng.random((K, T)).astype(np.float32)
    eng = Engine(0)
    for p, w in [(50, None), (20, None), (50, 1001), (20, 1000), (50, a.window), (20, a.window)]:
        eng.df_load(Yf)
        eng.profile(True); eng.profile_reset()
        torch.cuda.synchronize(); t0 = time.perf_counter()
        eng.df_finish(np.ones(K), p, w, Cm, Cm)
        wall = time.perf_counter() - t0
        tab = eng.profile_table()
        eng.profile(False)
        print(json.dumps(dict(what="baseline alone", K=K, T=T, df_prctile=p, df_window=w, finish_wall_ms=round(1e3 * wall, 2),
                              kernel_ms={k: round(v["total_ms"], 3) for k, v in tab.items() if k.startswith("df_")})), flush=True)
    eng.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="c3", choices=["c3", "c4", "tiny"])
    ap.add_argument("--host-route", action="store_true")
    ap.add_argument("--window", type=int, default=1000)
    ap.add_argument("--baseline-T", type=int, default=0, help="time the baseline kernels alone on K = 500 random-walk rows of this many frames (df_load + df_finish)")
    a = ap.parse_args()
    import torch
    if a.baseline_T:
        return baseline_only(a)
    from cnmf_e_amd import synth
    from cnmf_e_amd.engine import Engine
    from cnmf_e_amd.sources2d import PatchedVideo, Sources2D, Options
    d1, d2, T, K, r, seed = (96, 80, 400, 12, 6, 4) if a.config == "tiny" else (512, 512, 10000, 500, 15, 2)
    pdims = {"c3": [d1, d2], "c4": [128, 128], "tiny": [48, 40]}[a.config]
    f = synth.make_factors(d1, d2, T, K, seed)
    eng = Engine(0)
    if a.config != "c3":
        eng.set_option("lanes", 3)
    video = PatchedVideo(d1, d2, T, pdims, r, eng)
    for idx in video.owned:
        Yb = synth.make_video_device(f, "cuda:0", pixels=video.block_pix[idx])
        torch.cuda.synchronize()
        video.upload_block_device(idx, Yb.data_ptr())
        del Yb
    torch.cuda.empty_cache()
    s = Sources2D(video, Options(ring_radius=r, maxIter=5), f.A_init, f.C_init, f.sn)
    s.update_background_parallel(); s.update_spatial_parallel(); s.update_temporal_parallel()
    torch.cuda.synchronize()
    nnz = int(s.A.nnz)
    traffic = nnz * T * 4

    def emit(**kw):
        print(json.dumps(dict(config=a.config, d1=d1, d2=d2, T=T, K=int(s.A.shape[1]), patches=len(video.owned), **kw)), flush=True)

    groups = {"df_project": ("df_project",), "reconstruct": ("rss_const", "bg_reconstruct"), "df_scale": ("df_scale",), "df_base": ("df_base", "df_base_win"),
              "df_divide": ("df_divide",)}
    def timed():
        torch.cuda.synchronize(); t0 = time.perf_counter()
        s.extract_DF_F_endoscope()
        torch.cuda.synchronize()
        return time.perf_counter() - t0

    cold = timed()                                                         # (pays the allocations and the realisation of the residual the temporal update only recorded)
    emit(what="first call", wall_ms=round(1e3 * cold, 2))
    for p, w in [(50, None), (20, a.window)]:
        s.options.df_prctile, s.options.df_window = p, w
        walls = [timed() for _ in range(3)]                                # the profiler off: the end-to-end figure
        wall = sorted(walls)[1]
        eng.profile(True); eng.profile_reset()
        timed()                                                            # the phases: a run of their own (an event pair around every launch slows the host)
        tab = eng.profile_table()
        eng.profile(False)
        ph = {g: round(sum(tab.get(n, {}).get("total_ms", 0.0) for n in names), 3) for g, names in groups.items()}
        ph["residual_and_other"] = round(sum(v["total_ms"] for v in tab.values()) - sum(ph.values()), 3)
        proj_ms = ph["df_project"]
        emit(what="extract_DF_F_endoscope", df_prctile=p, df_window=w, wall_ms_median_of_3=round(1e3 * wall, 2), wall_ms_all=[round(1e3 * x, 2) for x in walls], kernel_ms=ph, nnz_A=nnz, df_project_algorithmic_bytes=traffic,
             df_project_TBps=round(traffic / (proj_ms * 1e-3) / 1e12, 3) if proj_ms else None, df_project_calls=tab.get("df_project", {}).get("calls", 0))
    if a.host_route:
        torch.cuda.synchronize(); t0 = time.perf_counter()
        Ybg = s.reconstruct_background()
        t1 = time.perf_counter()
        At = s.A.T.tocsr().astype(np.float32)
        Yf = np.asarray(At @ Ybg.reshape(d1 * d2, -1, order="F"), dtype=np.float64)
        t2 = time.perf_counter()
        Df = np.median(Yf / np.asarray(s.A.astype(np.float64).power(2).sum(axis=0)).ravel()[:, None], axis=1)
        t3 = time.perf_counter()
        emit(what="host route", reconstruct_to_host_ms=round(1e3 * (t1 - t0), 1), scipy_product_ms=round(1e3 * (t2 - t1), 1), median_ms=round(1e3 * (t3 - t2), 1),
             host_bytes=int(Ybg.nbytes), Df_mean=float(Df.mean()))
    eng.close()


if __name__ == "__main__":
    main()
