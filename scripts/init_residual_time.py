"""Times the OPEN of a residual peel session (cnmfe_peel_open_residual: the source pass k_peel_yres + the seed pipeline on the patch) next to the open of a block
session (cnmfe_peel_open) on the same patch, at the bench's scale: one 512 x 512 patch, a few thousand frames, the bench's neuron density.  Device time per kernel
(HIP events, cnmfe_profile_enable) and the wall time of each call, warmed up, median of `reps`.  A report, not a gate.

    python scripts/init_residual_time.py [--d 512] [--T 3000] [--K 500] [--reps 5]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

OPEN = ("seed_filter", "seed_stats", "seed_corr", "seed_cn", "peel_hy_final")


def run(d, T, K, reps, seed=2):
    import torch
    from cnmf_e_amd import synth
    from cnmf_e_amd.engine import Engine
    from cnmf_e_amd.sources2d import PatchedVideo, Sources2D, Options, seed_psf
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
        psf = seed_psf(3.0, 13.0, True)
        ind, A_blk = s._slice(s.A, idx, "block")
        C_blk = s._rows(s.C, ind)
        A_pp = s._slice(s.A, idx, "patch", cols=ind)[1]
        out = dict(d=d, T=T, K=int(ind.size), nnz_A=int(A_pp.nnz), video_bytes=16 * ((T + 3) // 4) * d * d)

        def timed(fn, names):
            walls, dev = [], []
            for rep in range(reps + 1):                       # the first repetition warms up (code objects, buffers)
                prep = fn(None)
                eng.synchronize()
                eng.profile(True); eng.profile_reset()
                t0 = time.perf_counter()
                fn(prep)
                eng.synchronize()
                walls.append(time.perf_counter() - t0)
                tab = eng.profile_table()
                eng.profile(False)
                dev.append({n: float(tab.get(n, {}).get("total_ms", 0.0)) for n in names})
                eng.peel_close(pid)
            walls, dev = walls[1:], dev[1:]
            return dict(wall_ms=1e3 * float(np.median(walls)), device_ms={n: float(np.median([x[n] for x in dev])) for n in names})

        def block(prep):
            if prep is None:
                return 1
            eng.peel_open(pid, psf)

        def resid(prep):
            if prep is None:                                  # the residual request and its realisation are not part of the open
                s._residual(idx, A_blk, C_blk)
                eng.get_sn(pid)
                return 1
            eng.peel_open_residual(pid, A_pp, C_blk, psf)

        out["peel_open"] = timed(block, OPEN)
        out["peel_open_residual"] = timed(resid, ("peel_yres",) + OPEN)
        y = out["peel_open_residual"]["device_ms"]["peel_yres"]
        out["peel_yres_GBps"] = 2 * out["video_bytes"] / (y * 1e-3) / 1e9 if y > 0 else None      # 16 B read + 16 B written per (pixel, frame quad)
        return out
    finally:
        eng.close()


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--d", type=int, default=512)
    ap.add_argument("--T", type=int, default=3000)
    ap.add_argument("--K", type=int, default=500)
    ap.add_argument("--reps", type=int, default=5)
    a = ap.parse_args()
    print(json.dumps(run(a.d, a.T, a.K, a.reps)))
