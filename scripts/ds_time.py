"""Times the down-sampled peel session (cnmfe_peel_open_ds, csrc/ds.hpp) beside the plain one at the headline block 512 x 512 x 10000: per (ssub, tsub) the wall
time of the open and of one extract + apply step around a planted neuron, and the device time of the ds kernels (HIP events, cnmfe_profile_enable).  Run under
`rocprofv3 --kernel-trace --stats -- python scripts/ds_time.py` for the per-kernel times DESIGN.md section 3 quotes.  A report, not a gate.

    python scripts/ds_time.py [--d 512] [--T 10000]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def run(d, T, nneur=50, seed=1):
    import torch
    from cnmf_e_amd import synth
    from cnmf_e_amd.engine import Engine
    from cnmf_e_amd.sources2d import PatchedVideo, seed_psf, bspline_basis, _mround
    f = synth.make_factors(d, d, T, nneur, seed)
    p0 = int(np.argmax(f.A_true[:, 0].toarray().ravel()))
    r0, c0 = p0 % d, p0 // d
    eng = Engine(0)
    out = dict(d=d, T=T, seed_pixel=(r0, c0), runs=[])
    try:
        eng.set_option("prealloc", 0)
        video = PatchedVideo(d, d, T, [d, d], 15, eng)
        Yb = synth.make_video_device(f, "cuda:0", pixels=video.block_pix[(0, 0)])
        video.upload_block_device((0, 0), Yb.data_ptr())
        eng.ymean(0)
        del Yb
        torch.cuda.empty_cache()
        Qpre = np.linalg.qr(bspline_basis(T, 3))[0]

        def step(r, c, g):
            t0 = time.perf_counter()
            corr, ai, ci, st = eng.peel_extract(0, r, c, g)
            t1 = time.perf_counter()
            n, nr, nc = eng._peel[0]
            a0, a1, b0, b1 = eng.peel_box(nr, nc, r, c, g)
            s0, s1, u0, u1 = eng.peel_box(nr, nc, r, c, 2 * g)
            big = np.zeros((s1 - s0, u1 - u0)); big[a0 - s0:a1 - s0, b0 - u0:b1 - u0] = ai
            eng.peel_apply(0, r, c, g, ai, big, np.nan_to_num(ci), 3.0, 8.0, 0.8)
            return (t1 - t0) * 1e3, (time.perf_counter() - t1) * 1e3

        for rep in range(2):                                  # the second round is the one reported (the first pays the one-off set-up of every kernel)
            runs = []
            for (ssub, tsub, Q) in ((0, 0, None), (2, 1, None), (1, 5, None), (2, 5, None), (2, 5, Qpre)):
                eng.profile(True); eng.profile_reset()
                g = int(_mround(13.0 / max(ssub, 1)))
                psf = seed_psf(3.0 / max(ssub, 1), float(g), True)
                t0 = time.perf_counter()
                if ssub == 0:
                    eng.peel_open(0, psf, T, None, 3.0)
                else:
                    eng.peel_open_ds(0, ssub, tsub, psf, T, Q, 3.0)
                t_open = (time.perf_counter() - t0) * 1e3
                t_ex, t_ap = step(r0 // max(ssub, 1), c0 // max(ssub, 1), g)
                eng.peel_close(0)
                tab = eng.profile_table()
                eng.profile(False)
                runs.append(dict(ssub=ssub, tsub=tsub, Mpre=0 if Q is None else int(Q.shape[1]), open_ms=t_open, extract_ms=t_ex, apply_ms=t_ap,
                                 device_ms={k: round(v["total_ms"], 4) for k, v in tab.items() if k.startswith("ds_")}))
            out["runs"] = runs
        return out
    finally:
        eng.close()


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--d", type=int, default=512)
    ap.add_argument("--T", type=int, default=10000)
    a = ap.parse_args()
    print(json.dumps(run(a.d, a.T)))
