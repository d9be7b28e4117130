"""Times the two calls background_model = 'svd' gained, at the bench's scale (one 512 x 512 patch, 3000 frames, nb = 1, the bench's K = 500):

  * cnmfe_peel_open_lowrank, the whole call and its source kernel k_peel_yres_lowrank, against the two-step route on the same build,
    cnmfe_residual_lowrank (k_lowrank_resid) followed by cnmfe_peel_open_residual (k_peel_yres) -- the two routes alternate inside one loop;
  * cnmfe_demix_frames_lowrank for 100 displayed frames against cnmfe_demix_frames on a ring-mode object of the same size.

Wall times are host clocks around a call that ends in a device synchronise; kernel times are the engine's HIP-event profile.  Each figure is the mean of `reps`
runs after one warm-up run, with its smallest and largest run beside it (the spread).  A report, not a gate: it writes profiles/svd_second_pass/probe.json.

    python scripts/svd_second_pass_probe.py [--d 512] [--T 3000] [--K 500] [--reps 10] [--out profiles/svd_second_pass/probe.json]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SEED_KERNELS = ("seed_filter", "seed_stats", "seed_corr", "seed_cn", "peel_hy_final")


def _stat(xs):
    xs = [float(x) for x in xs]
    return dict(mean=float(np.mean(xs)), min=min(xs), max=max(xs))


def _timed(eng, fn, names):
    """one profiled, synchronised run of fn: (wall ms, device ms per kernel name)"""
    eng.synchronize()
    eng.profile(True); eng.profile_reset()
    t0 = time.perf_counter()
    fn()
    eng.synchronize()
    wall = 1e3 * (time.perf_counter() - t0)
    tab = eng.profile_table()
    eng.profile(False)
    return wall, {n: float(tab.get(n, {}).get("total_ms", 0.0)) for n in names}


def _object(eng, f, d, T, svd):
    import torch
    from cnmf_e_amd import synth
    from cnmf_e_amd.sources2d import PatchedVideo, Sources2D, Options
    video = PatchedVideo(d, d, T, [d, d], 15, eng)
    idx = video.owned[0]
    Yb = synth.make_video_device(f, "cuda:0", pixels=video.block_pix[idx])
    video.upload_block_device(idx, Yb.data_ptr())
    eng.ymean(video.pid[idx])
    del Yb
    torch.cuda.empty_cache()
    opts = Options(ring_radius=15, gSig=3, gSiz=13, background_model="svd", nb=1) if svd else Options(ring_radius=15, gSig=3, gSiz=13)
    return video, idx, Sources2D(video, opts, f.A_init, f.C_init, f.sn)


def run(d, T, K, reps, nframes=100, seed=2):
    import torch                                                     # (before the engine's library: the order scripts/init_residual_time.py and bench.py load them in)
    from cnmf_e_amd import synth
    from cnmf_e_amd.engine import Engine
    from cnmf_e_amd.sources2d import seed_psf
    f = synth.make_factors(d, d, T, K, seed)
    psf = seed_psf(3.0, 13.0, True)
    out = dict(d=d, T=T, nb=1, reps=reps, video_bytes=16 * ((T + 3) // 4) * d * d, demix_frames=nframes)
    stride = max(1, (T - 1) // max(nframes - 1, 1))

    eng = Engine(0)
    try:
        video, idx, s = _object(eng, f, d, T, True)
        pid = video.pid[idx]
        s.update_background_parallel()                              # the fit: b, f, b0 of the patch
        ind, A_pp = s._slice(s.A, idx, "patch")
        C_p = s._rows(s.C, ind)
        out.update(K=int(ind.size), nnz_A=int(A_pp.nnz))
        fused_names = ("peel_yres_lowrank",) + SEED_KERNELS
        two_names = ("lowrank_resid", "peel_yres") + SEED_KERNELS

        def fused():
            eng.peel_open_lowrank(pid, 1, 1, A_pp, C_p, psf)

        def two_step():
            eng.residual_lowrank(pid)
            eng.peel_open_residual(pid, A_pp, C_p, psf)

        rec = {"fused": [], "two_step": []}
        for rep in range(reps + 1):                                 # the first repetition warms up; the routes alternate
            for name, fn, names in (("fused", fused, fused_names), ("two_step", two_step, two_names)):
                eng.bg_svd_set(pid, *eng.bg_svd_get(pid))           # drops the resident residual: the two-step route realises it every time
                rec[name].append(_timed(eng, fn, names))
                eng.peel_close(pid)
        for name, names in (("fused", fused_names), ("two_step", two_names)):
            runs = rec[name][1:]
            out["open_" + name] = dict(wall_ms=_stat([w for w, _ in runs]), device_ms={n: _stat([dv[n] for _, dv in runs]) for n in names})
        y = out["open_fused"]["device_ms"]["peel_yres_lowrank"]["mean"]
        out["peel_yres_lowrank_GBps"] = 2 * out["video_bytes"] / (y * 1e-3) / 1e9 if y > 0 else None      # 16 B read + 16 B written per (pixel, frame quad)
        src2 = out["open_two_step"]["device_ms"]
        out["two_step_source_ms"] = src2["lowrank_resid"]["mean"] + src2["peel_yres"]["mean"]

        CC = s.C
        col = np.ones((ind.size, 3), np.float32)

        def demix_svd():
            eng.demix_frames_lowrank(pid, A_pp, CC, ind, col, 1000.0, 0, stride, nframes)
        runs = [_timed(eng, demix_svd, ("demix_panels_lowrank",)) for _ in range(reps + 1)][1:]
        out["demix_lowrank"] = dict(wall_ms=_stat([w for w, _ in runs]), device_ms=_stat([dv["demix_panels_lowrank"] for _, dv in runs]))
    finally:
        eng.close()

    eng = Engine(0)                                                  # the ring-mode object of the same size, on an engine of its own
    try:
        video, idx, s = _object(eng, f, d, T, False)
        pid = video.pid[idx]
        s.update_background_parallel()
        s._temporal_residual_early(idx)                              # the residual of (A_prev, C_prev), as demixed_frames requests it
        ind, A_pp = s._slice(s.A, idx, "patch")
        b0_ = s.reconstruct_b0().reshape(-1, order="F")
        b0n = np.asarray(s.b0_new, dtype=np.float64).reshape(-1, order="F")
        CC = s.C
        col = np.ones((ind.size, 3), np.float32)

        def demix_ring():
            eng.demix_frames(pid, b0_[video.block_pix[idx]], b0n[video.patch_pix[idx]], A_pp, CC, ind, col, 1000.0, 0, stride, nframes)
        runs = [_timed(eng, demix_ring, ("demix_panels",)) for _ in range(reps + 1)][1:]
        out["demix_ring"] = dict(wall_ms=_stat([w for w, _ in runs]), device_ms=_stat([dv["demix_panels"] for _, dv in runs]))
    finally:
        eng.close()
    return out


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--d", type=int, default=512)
    ap.add_argument("--T", type=int, default=3000)
    ap.add_argument("--K", type=int, default=500)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "svd_second_pass", "probe.json"))
    a = ap.parse_args()
    res = run(a.d, a.T, a.K, a.reps)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(res, fh, indent=1, sort_keys=True)
        fh.write("\n")
    print(json.dumps(res))
