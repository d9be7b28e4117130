"""initTemporal under background_model = 'svd' (cnmfe_init_temporal_lowrank) at one 512 x 512 x 3000 patch, K = 500, nb = 1: where the time of a call goes, the
reads of the video, and the projection's effective bandwidth beside the ring branch's init_temporal on the same recording ("Known footprints
under the low-rank background"; section 8 for the errors).

    python scripts/svd_init_temporal_probe.py [--reps 10] [--warmup 2] [--small] [--out profiles/svd_init_temporal/probe.json]

The video is synthesised in HBM (cnmf_e_amd.synth) once per model; one background update gives b (svd) or W, b0 (ring); every timed call is fenced by a
synchronize.  Wall times are means of --reps calls; the phases come from the engine's own kernel events in calls of their own (the events cost a few microseconds
per launch: those calls are not the timed ones), also means of --reps.  No threshold is set anywhere: the numbers are a record.  --parity adds the errors against
the float64 oracle on the small cases of tests/svd_init_temporal_cases.py (what tests/test_gpu_svd_init_temporal.py bounds)."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HBM_PEAK = 8.0e12            # bytes / s, MI355X
FP64_MATRIX_PEAK = 78.6e12   # flop / s, MI355X (v_mfma_f64_16x16x4_f64)
PHASES = {"gram": ("itl_gram", "itl_colconst"), "projection": ("temporal_build_B", "temporal_tile_video", "temporal_proj_B", "itl_reduce_R"),
          "solve": ("itl_trsm_forward", "itl_trsm_backward"), "finish": ("itl_finish", "itl_b0"), "sweeps": ("temporal_hals_level", "temporal_hals_deconv_level")}


def parity():
    for p in (os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests")):
        sys.path.insert(0, p)
    import svd_init_temporal_cases as sic
    import test_gpu_svd_init_temporal as t
    from parity_util import rel
    out = {}
    for name in sorted(sic.CASES):
        ref = sic.reference(name)
        with t.Run(name) as r:
            r.s.initTemporal()
            ef, es, eb = t._factor_errors(r, ref)
            out[name] = dict(C_raw=rel(np.asarray(r.s.C_raw, dtype=np.float32), ref["C_raw"]), f=ef, f_stored_video=es, b0=eb,
                             video_reads=r.eng.counter("init_temporal_lowrank_video_reads"))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--small", action="store_true", help="128 x 128 x 1000, K = 40: a dry run of the script")
    ap.add_argument("--parity", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    from cnmf_e_amd import synth
    from cnmf_e_amd.engine import Engine
    from cnmf_e_amd.sources2d import PatchedVideo, Sources2D, Options
    d1, d2, T, K, r = (128, 128, 1000, 40, 15) if a.small else (512, 512, 3000, 500, 15)
    f = synth.make_factors(d1, d2, T, K, 1)
    A = f.A_true.astype(np.float32)

    def make(model):
        eng = Engine(0)
        video = PatchedVideo(d1, d2, T, [d1, d2], r, eng)
        for idx in video.owned:
            Yb = synth.make_video_device(f, "cuda:0", pixels=video.block_pix[idx])
            torch.cuda.synchronize()
            video.upload_block_device(idx, Yb.data_ptr())
            del Yb
        torch.cuda.empty_cache()
        s = Sources2D(video, Options(ring_radius=r, maxIter=5, background_model=model, nb=1), A, f.C_init, f.sn)
        s.update_background_parallel()
        if model == "svd":                                                 # the fitted factors, handed back: initTemporal extracts under a background it is GIVEN
            for idx in video.owned:
                s.set_bg_svd(idx, s.get_b(idx), s.get_f(idx), s.get_b0(idx))
        eng.synchronize()
        return eng, video, s

    def timed(eng, fn):
        eng.synchronize()
        t0 = time.perf_counter()
        fn()
        eng.synchronize()
        return (time.perf_counter() - t0) * 1e3

    def run(model):
        eng, video, s = make(model)
        for _ in range(a.warmup):
            timed(eng, s.initTemporal)
        wall = [timed(eng, s.initTemporal) for _ in range(a.reps)]
        eng.profile(True)
        factor_us = []
        for _ in range(a.reps):
            timed(eng, s.initTemporal)
            if model == "svd":
                factor_us.append(eng.counter("init_temporal_lowrank_factor_us"))
        tab = {k: v for k, v in eng.profile_table().items() if v["calls"]}
        eng.profile(False)
        kern = {k: v["total_ms"] / a.reps for k, v in tab.items()}
        d_b = sum(video.block_pix[idx].size for idx in video.owned)
        out = dict(wall_ms_mean=float(np.mean(wall)), wall_ms_all=[round(x, 3) for x in wall], kernels_ms={k: round(v, 4) for k, v in sorted(kern.items(), key=lambda kv: -kv[1])[:16]},
                   launches_per_call={k: v["calls"] / a.reps for k, v in tab.items() if k in ("temporal_proj_B", "temporal_build_B", "temporal_hals_level")})
        proj = kern.get("temporal_proj_B")
        out["proj_B_ms"] = proj
        out["proj_effective_bytes_per_s"] = 4.0 * d_b * T / (proj * 1e-3) if proj else None
        out["proj_hbm_fraction"] = out["proj_effective_bytes_per_s"] / HBM_PEAK if proj else None
        if model == "svd":
            out["phases_ms"] = {p: round(sum(kern.get(k, 0.0) for k in names), 4) for p, names in PHASES.items()}
            out["phases_ms"]["host_factorisation"] = round(float(np.mean(factor_us)) * 1e-3, 4)
            out["video_reads"] = eng.counter("init_temporal_lowrank_video_reads")
            n = K + 1
            n16 = (n + 15) // 16 * 16
            flops = 2.0 * 2.0 * (n16 * n16 / 2.0) * (-(-T // 64) * 64)        # two triangular solves, n16^2 / 2 multiply-adds per column each
            solve = out["phases_ms"]["solve"]
            out["solve_flops"] = flops
            out["solve_fraction_of_fp64_matrix_peak"] = flops / (solve * 1e-3) / FP64_MATRIX_PEAK if solve else None
            out["unknowns"] = n
        eng.close()
        return out

    res = {"size": [d1, d2, T, K, r], "nb": 1, "reps": a.reps, "svd": run("svd"), "ring": run("ring")}
    if a.parity:
        res["parity_observed"] = parity()
    txt = json.dumps(res, indent=1, sort_keys=True)
    print(txt)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write(txt + "\n")


if __name__ == "__main__":
    main()
