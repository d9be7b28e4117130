"""Time of one Sources2D.initTemporal at the bench size (512 x 512 x 10000, K = 500, r = 15; DESIGN.md section 3, "(f) known footprints"), with
update_temporal_parallel of the same build at the same size beside it as the yardstick.

    python scripts/init_temporal_time.py [--reps 5] [--warmup 2] [--deconv] [--small] [--once]

The video is synthesised in HBM (cnmf_e_amd.synth), one background fit gives W and b0, then the two methods ALTERNATE (a warm-up of each first); every call is
fenced by a synchronize.  Prints one JSON line: medians in ms, the level count of initTemporal's schedule, the (block, column) entries of its projection and --
from the engine's own kernel events, in a pass of their own after the timed ones -- the projection's time and its fraction of the HBM roofline.  --once: a
single initTemporal after the fit and nothing else (the shape of a `rocprofv3 --kernel-trace --stats -- python scripts/init_temporal_time.py --once` run)."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

HBM_PEAK = 8.0e12            # bytes / s, MI355X


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--deconv", action="store_true")
    ap.add_argument("--small", action="store_true", help="128 x 128 x 2000, K = 40: a dry run of the script")
    ap.add_argument("--once", action="store_true")
    a = ap.parse_args()
    import torch
    from cnmf_e_amd import synth
    from cnmf_e_amd.engine import Engine
    from cnmf_e_amd.sources2d import PatchedVideo, Sources2D, Options
    d1, d2, T, K, r = (128, 128, 2000, 40, 15) if a.small else (512, 512, 10000, 500, 15)
    f = synth.make_factors(d1, d2, T, K, 1)
    eng = Engine(0)
    video = PatchedVideo(d1, d2, T, [d1, d2], r, eng)
    for idx in video.owned:
        Yb = synth.make_video_device(f, "cuda:0", pixels=video.block_pix[idx])
        torch.cuda.synchronize()
        video.upload_block_device(idx, Yb.data_ptr())
        del Yb
    torch.cuda.empty_cache()
    s = Sources2D(video, Options(ring_radius=r, maxIter=5, deconv_flag=a.deconv), f.A_true.astype(np.float32), f.C_init, f.sn)
    s.update_background_parallel()
    eng.synchronize()

    def timed(fn):
        eng.synchronize()
        t0 = time.perf_counter()
        fn()
        eng.synchronize()
        return (time.perf_counter() - t0) * 1e3

    if a.once:
        print(json.dumps({"init_temporal_ms": timed(s.initTemporal), "levels": eng.counter("init_temporal_levels")}))
        return
    init = lambda: s.initTemporal()

    def upd():
        s.update_temporal_parallel()

    for _ in range(a.warmup):
        timed(init); timed(upd)
    ti, tu = [], []
    for _ in range(a.reps):
        ti.append(timed(init)); tu.append(timed(upd))
    levels, entries = eng.counter("init_temporal_levels"), None
    eng.profile(True)
    timed(init)
    entries = eng.counter("temporal_proj_entries")
    tab = {k: v for k, v in eng.profile_table().items() if v["calls"]}
    eng.profile(False)
    proj = tab.get("temporal_proj_B", {"total_ms": float("nan"), "calls": 0})
    d_b = sum(video.block_pix[idx].size for idx in video.owned)
    bytes_video = 4.0 * d_b * T                      # fp32 tiles (the int8 planes of a video a fit has touched hold as many bytes: 4 planes x 1 byte)
    out = {"size": [d1, d2, T, K, r], "deconv": bool(a.deconv), "init_temporal_ms": float(np.median(ti)), "init_temporal_all_ms": [round(x, 3) for x in ti],
           "update_temporal_ms": float(np.median(tu)), "update_temporal_all_ms": [round(x, 3) for x in tu], "levels": int(levels), "proj_entries": int(entries),
           "proj_ms": proj["total_ms"], "proj_launches": proj["calls"], "proj_hbm_fraction": bytes_video / (proj["total_ms"] * 1e-3) / HBM_PEAK if proj["calls"] else None,
           "kernels_ms": {k: round(v["total_ms"], 4) for k, v in sorted(tab.items(), key=lambda kv: -kv[1]["total_ms"])[:14]}}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
