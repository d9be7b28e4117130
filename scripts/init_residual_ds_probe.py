"""Times the OPEN of the down-sampled residual peel session (cnmfe_peel_open_residual_ds: the source pass k_ds_video_res, the bin means k_trace_bin_mean, the seed
pipeline on the low-resolution grid) at the bench's scale: one 512 x 512 patch, 3000 frames, the bench's neuron density, for the factor pairs (ssub, tsub) =
(1, 1), (2, 1), (1, 5), (2, 5).  (1, 1) is cnmfe_peel_open_residual itself -- the comparison.  Per pair: the wall time of the call (host clock around work that
ends in a device synchronise) and the device time per kernel (the library's own HIP events, cnmfe_profile_enable), MEANS of `reps` repetitions after one warm-up
of every shape, the pairs visited in turn within every repetition so that drift of a shared host hits them alike; and the session's device bytes,
2 x 16 ceil(Ts / 4) d1s d2s.  A report, not a gate.

    python scripts/init_residual_ds_probe.py [--d 512] [--T 3000] [--K 500] [--reps 10] [--out profiles/init_residual_ds/probe.json]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

PAIRS = ((1, 1), (2, 1), (1, 5), (2, 5))
SEED = ("seed_filter", "seed_stats", "seed_corr", "seed_cn", "peel_hy_final")
SOURCE = ("peel_yres", "ds_video_res", "trace_bin_mean")


def run(d, T, K, reps, seed=2):
    import torch
    from cnmf_e_amd import synth
    from cnmf_e_amd.engine import Engine
    from cnmf_e_amd.sources2d import PatchedVideo, Sources2D, Options, seed_psf, _mround
    if not torch.cuda.is_available():
        raise SystemExit("init_residual_ds_probe: no GPU -- nothing is measured without one")
    f = synth.make_factors(d, d, T, K, seed)
    eng = Engine(0)
    try:
        video = PatchedVideo(d, d, T, [d, d], 15, eng)
        idx = video.owned[0]
        pid = video.pid[idx]
        Yb = synth.make_video_device(f, "cuda:0", pixels=video.block_pix[idx])
        video.upload_block_device(idx, Yb.data_ptr())
        eng.ymean(pid)
        del Yb
        torch.cuda.empty_cache()
        s = Sources2D(video, Options(ring_radius=15, gSig=3, gSiz=13), f.A_init, f.C_init, f.sn)
        s.update_background_parallel()
        ind, A_blk = s._slice(s.A, idx, "block")
        C_blk = s._rows(s.C, ind)
        A_pp = s._slice(s.A, idx, "patch", cols=ind)[1]
        out = dict(d=d, T=T, K=int(ind.size), nnz_A=int(A_pp.nnz), reps=reps, pairs={})
        names = SOURCE + SEED
        walls = {p: [] for p in PAIRS}
        dev = {p: [] for p in PAIRS}
        for rep in range(reps + 1):                               # the first repetition warms every shape up (code objects, buffers)
            for (ssub, tsub) in PAIRS:
                psf = seed_psf(3.0 / ssub, float(_mround(13.0 / ssub)), True)
                s._residual(idx, A_blk, C_blk)                    # the residual request and its realisation are not part of the open
                eng.get_sn(pid)
                eng.synchronize()
                eng.profile(True); eng.profile_reset()
                t0 = time.perf_counter()
                eng.peel_open_residual_ds(pid, ssub, tsub, A_pp, C_blk, psf)
                eng.synchronize()
                w = time.perf_counter() - t0
                tab = eng.profile_table()
                eng.profile(False)
                eng.peel_close(pid)
                if rep:
                    walls[(ssub, tsub)].append(w)
                    dev[(ssub, tsub)].append({n: float(tab.get(n, {}).get("total_ms", 0.0)) for n in names})
        for (ssub, tsub) in PAIRS:
            d1s, Ts = -(-d // ssub), T // tsub
            w = np.asarray(walls[(ssub, tsub)])
            dm = {n: float(np.mean([x[n] for x in dev[(ssub, tsub)]])) for n in names}
            src = dm["peel_yres"] + dm["ds_video_res"]
            out["pairs"]["%d,%d" % (ssub, tsub)] = dict(
                wall_ms_mean=1e3 * float(w.mean()), wall_ms_min=1e3 * float(w.min()), wall_ms_max=1e3 * float(w.max()),
                device_ms={n: v for n, v in dm.items() if v > 0}, seed_pipeline_ms=float(sum(dm[n] for n in SEED)), source_kernel_ms=src,
                session_bytes=2 * 16 * ((Ts + 3) // 4) * d1s * d1s, grid=[d1s, d1s, Ts],
                # the source pass reads the resident residual once (16 B per pixel and input frame quad) and writes the session's video
                source_GBps=(16 * ((T + 3) // 4) * d * d + 16 * ((Ts + 3) // 4) * d1s * d1s) / (src * 1e-3) / 1e9 if src > 0 else None)
        return out
    finally:
        eng.close()


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--d", type=int, default=512)
    ap.add_argument("--T", type=int, default=3000)
    ap.add_argument("--K", type=int, default=500)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "init_residual_ds", "probe.json"))
    a = ap.parse_args()
    res = run(a.d, a.T, a.K, a.reps)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(res, fh, indent=1, sort_keys=True)
    print(json.dumps(res))
