"""Times Sources2D.correlation_pnr_parallel (cnmfe_seed_images) per kernel with HIP events (cnmfe_profile_enable): the headline recording 512 x 512 x 10000,
gSig = 3 (113 taps), as ONE block and as the 4 x 4-patch split, against the bytes each kernel has to move (filter: read + write the block, stats and
correlation: read the filtered block once each), and the float64 oracle's host time at 128 x 128 x 3000 scaled by d * T as BASELINE.md section 3 scales.
A report, not a gate: there is no earlier number to compare with.

    python scripts/seed_images_time.py [--d 512] [--T 10000] [--gSig 3] [--nk 1] [--no-oracle]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
HBM_GBS = 8000.0          # MI355X peak HBM bandwidth the shares are quoted against


def run(d, T, pdims, gSig, nk, r=15, seed=1):
    import torch
    from cnmf_e_amd import synth
    from cnmf_e_amd.engine import Engine
    from cnmf_e_amd.sources2d import PatchedVideo, Sources2D, Options
    f = synth.make_factors(d, d, T, 8, seed)
    eng = Engine(0)
    try:
        eng.set_option("prealloc", 0)                         # no fit follows: the ring fit's buffers stay unallocated
        if pdims[0] < d:
            eng.set_option("lanes", 2)
        video = PatchedVideo(d, d, T, pdims, r, eng)
        for idx in video.owned:
            Yb = synth.make_video_device(f, "cuda:0", pixels=video.block_pix[idx])
            video.upload_block_device(idx, Yb.data_ptr())
            eng.ymean(video.pid[idx])                       # the resident centred copy is built here, not inside the timed call
            del Yb
        torch.cuda.empty_cache()
        s = Sources2D(video, Options(ring_radius=r, gSig=gSig, gSiz=4 * gSig + 1, nk=nk), f.A_init, f.C_init, f.sn)
        s.correlation_pnr_parallel()                         # warm: code objects, the first allocation
        eng.profile(True); eng.profile_reset()
        t0 = time.perf_counter()
        Cn, PNR = s.correlation_pnr_parallel()
        wall = time.perf_counter() - t0
        tab = eng.profile_table()
        eng.profile(False)
        d_b = sum(video.block_pix[idx].size for idx in video.owned)
        blk = 16.0 * ((T + 3) // 4) * d_b                    # one float4-interleaved copy of all blocks
        out = dict(d=d, T=T, patches=len(video.owned), gSig=gSig, nk=nk, wall_s=wall, block_bytes=blk, kernels={})
        for name, nbytes in (("seed_filter", 2 * blk), ("seed_stats", blk), ("seed_corr", blk), ("seed_cn", 0.0)):
            ms = tab.get(name, {}).get("total_ms", float("nan"))
            out["kernels"][name] = dict(ms=ms, gbytes=nbytes / 1e9, gbs=nbytes / ms / 1e6 if ms == ms and ms > 0 else None,
                                        frac_of_hbm=nbytes / ms / 1e6 / HBM_GBS if ms == ms and ms > 0 else None)
        out["finite"] = bool(np.all(np.isfinite(Cn)) and np.all(np.isfinite(PNR)))
        return out
    finally:
        eng.close()


def oracle_time(gSig):
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import seed_oracle as so
    from cnmf_e_amd import synth
    d, T = 128, 3000
    f = synth.make_factors(d, d, T, 31, 9)
    Y = synth.make_video(f, np.float32)
    t0 = time.perf_counter()
    so.seed_images(Y.T.astype(np.float64), d, d, gSig, 4 * gSig + 1)
    return d, T, time.perf_counter() - t0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--d", type=int, default=512)
    ap.add_argument("--T", type=int, default=10000)
    ap.add_argument("--gSig", type=float, default=3.0)
    ap.add_argument("--nk", type=int, default=1)
    ap.add_argument("--no-oracle", action="store_true")
    a = ap.parse_args()
    res = []
    for pd in ([a.d, a.d], [a.d // 4, a.d // 4]):
        o = run(a.d, a.T, pd, a.gSig, a.nk)
        res.append(o)
        print("%d x %d x %d, %d patch(es), gSig %g, nk %d: call %.1f ms wall" % (a.d, a.d, a.T, o["patches"], a.gSig, a.nk, 1e3 * o["wall_s"]))
        for k, v in o["kernels"].items():
            if v["gbs"] is not None:
                print("  %-12s %9.2f ms   %6.2f GB   %7.0f GB/s  = %4.1f %% of HBM peak" % (k, v["ms"], v["gbytes"], v["gbs"], 100 * v["frac_of_hbm"]))
            else:
                print("  %-12s %9.2f ms" % (k, v["ms"]))
    if not a.no_oracle:
        od, oT, ot = oracle_time(a.gSig)
        scaled = ot * (a.d * a.d * a.T) / float(od * od * oT)
        print("float64 oracle on the host: %.1f s at %d x %d x %d -> %.0f s scaled by d * T to %d x %d x %d" % (ot, od, od, oT, scaled, a.d, a.d, a.T))
        res.append(dict(oracle_s=ot, oracle_d=od, oracle_T=oT, oracle_scaled_s=scaled))
    print(json.dumps(res))


if __name__ == "__main__":
    main()
