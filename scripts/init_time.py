"""Times one Sources2D.initComponents_parallel (the peel session of csrc/peel.hpp + the host loop of hostops.greedy_roi_block) at the headline recording
512 x 512 x 10000 with the demo's parameters (gSig 3, gSiz 13, min_corr 0.8, min_pnr 8: demo_large_data_1p.m:45-50), and prints the device time per phase
(HIP events, cnmfe_profile_enable), the wall time and the number of neurons.  A report, not a gate: there is no earlier number to compare with.

    python scripts/init_time.py [--d 512] [--T 10000] [--K 0] [--patch 0]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

PHASES = {"open": ("seed_filter", "seed_stats", "seed_corr", "seed_cn", "peel_hy_final", "peel_yw_detrend"),
          "extract": ("peel_corr_part", "peel_corr_fin", "peel_traces", "peel_trace_stats", "peel_mom_part", "peel_ai_fin"),
          "apply": ("peel_rank1_yw", "peel_rank1_hy", "peel_box_part", "peel_box_rec", "peel_corr8", "peel_cn")}


def run(d, T, K, patch, nneur=200, seed=1):
    import torch
    from cnmf_e_amd import synth
    from cnmf_e_amd.engine import Engine
    from cnmf_e_amd.sources2d import PatchedVideo, Sources2D, Options
    f = synth.make_factors(d, d, T, nneur, seed)
    eng = Engine(0)
    try:
        eng.set_option("prealloc", 0)                         # no fit follows: the ring fit's buffers stay unallocated
        video = PatchedVideo(d, d, T, [patch or d, patch or d], 15, eng)
        for idx in video.owned:
            Yb = synth.make_video_device(f, "cuda:0", pixels=video.block_pix[idx])
            video.upload_block_device(idx, Yb.data_ptr())
            eng.ymean(video.pid[idx])
            del Yb
        torch.cuda.empty_cache()
        s = Sources2D(video, Options(ring_radius=15, gSig=3, gSiz=13, min_corr=0.8, min_pnr=8.0, bd=None), f.A_init, f.C_init, f.sn)
        eng.profile(True); eng.profile_reset()
        t0 = time.perf_counter()
        center, Cn, PNR = s.initComponents_parallel(K=K or None)
        wall = time.perf_counter() - t0
        tab = eng.profile_table()
        eng.profile(False)
        out = dict(d=d, T=T, patches=len(video.owned), planted=nneur, neurons=int(center.shape[0]), wall_s=wall, device_ms={}, calls={})
        for ph, names in PHASES.items():
            out["device_ms"][ph] = float(sum(tab.get(n, {}).get("total_ms", 0.0) for n in names))
        out["calls"] = {ph: int(tab.get(n, {}).get("calls", 0)) for ph, n in (("extract", "peel_corr_part"), ("apply", "peel_cn"))}
        out["host_s"] = wall - sum(out["device_ms"].values()) / 1e3
        return out
    finally:
        eng.close()


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--d", type=int, default=512)
    ap.add_argument("--T", type=int, default=10000)
    ap.add_argument("--K", type=int, default=0, help="cap on the neurons per patch (0: none)")
    ap.add_argument("--patch", type=int, default=0, help="patch size (0: one patch)")
    ap.add_argument("--neurons", type=int, default=200, help="neurons planted in the synthetic recording")
    a = ap.parse_args()
    print(json.dumps(run(a.d, a.T, a.K, a.patch, a.neurons)))
