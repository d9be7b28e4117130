"""Times of the low-rank background (background_model = 'svd') on one patch: python scripts/svd_bg_probe.py [--out profiles/svd_bg/probe.json]

512 x 512 x 3000 with the bench's K = 500, and the headline size 512 x 512 x 10000 if the free device memory allows (checked before the size is started; an error of a started size ends the script).  Per size: the two video passes of one iteration
(k_svd_project, k_svd_expand) against the bytes they read at the HBM rate the projections reach (README: 4.3 - 4.4 TB/s), the passes and iterations to converge, the
whole fit (wall clock around the blocking call), and k_lowrank_resid (one read of the block video, one write of the patch).  Recorded, not gated: a new kernel has no
parent to compare with.  For context the steady-state ring fit of the headline size from profiles/r06 (bench_c3_v9.json) is copied beside them."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HBM_PROJ_TBS = 4.35


def run(eng, d1, d2, T, K, nb, seed):
    import torch
    from cnmf_e_amd import synth
    from cnmf_e_amd.sources2d import PatchedVideo
    f = synth.make_factors(d1, d2, T, K, seed)
    video = PatchedVideo(d1, d2, T, [d1, d2], 15, eng)
    idx = video.order[0]; pid = video.pid[idx]
    if torch.cuda.is_available():                              # synthesised in HBM, as bench.py does
        Yb = synth.make_video_device(f, "cuda:0", pixels=video.block_pix[idx])
        torch.cuda.synchronize()
        video.upload_block_device(idx, Yb.data_ptr())
        del Yb
        torch.cuda.empty_cache()
    else:                                                      # ... or on the host, where torch sees no device
        video.upload_from_full(synth.make_video(f, np.float32))
    eng.ymean(pid)
    A = f.A_init.tocsc().astype(np.float32); C = np.ascontiguousarray(f.C_init, dtype=np.float32)
    eng.bind_traces(C)
    eng.bg_svd_fit(pid, nb, A, C)                              # warm: allocations, code objects
    eng.synchronize()
    eng.profile(True); eng.profile_reset()
    t0 = time.perf_counter()
    st = eng.bg_svd_fit(pid, nb, A, C)
    eng.synchronize()
    fit_ms = (time.perf_counter() - t0) * 1e3
    tab = eng.profile_table()
    eng.profile_reset()
    eng.residual_lowrank(pid)
    eng.synchronize()
    tab2 = eng.profile_table()
    eng.profile(False)
    vbytes = d1 * d2 * ((T + 3) // 4) * 16
    per = lambda n, t=tab: t[n]["total_ms"] / max(1, t[n]["calls"])
    out = dict(d1=d1, d2=d2, T=T, K=K, nb=nb, video_bytes=vbytes, hbm_floor_ms_per_pass=vbytes / (HBM_PROJ_TBS * 1e12) * 1e3,
               project_ms=per("svd_project"), expand_ms=per("svd_expand"), rowsum_ms=per("svd_rowsum"),
               project_TBs=vbytes / per("svd_project") / 1e9, expand_TBs=vbytes / per("svd_expand") / 1e9,
               iterations=st["iterations"], passes=st["passes"], converged=st["converged"], residual=[float(x) for x in st["residual"]],
               fit_wall_ms=fit_ms, fit_kernels_ms=sum(v["total_ms"] for v in tab.values()),
               kernels_ms={k: round(v["total_ms"], 4) for k, v in sorted(tab.items()) if k.startswith("svd") or k in ("center_traces",)},
               lowrank_resid_ms=per("lowrank_resid", tab2), lowrank_resid_TBs=2 * vbytes / per("lowrank_resid", tab2) / 1e9)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "svd_bg", "probe.json"))
    ap.add_argument("--nb", type=int, default=1)
    a = ap.parse_args()
    import torch
    from cnmf_e_amd.engine import Engine
    if torch.cuda.is_available():                              # (torch first, as in bench.py)
        torch.cuda.set_device(0)
    res = {"hbm_rate_of_the_projections_TBs": HBM_PROJ_TBS, "sizes": []}
    for (d1, d2, T, K) in [(512, 512, 3000, 500), (512, 512, 10000, 500)]:
        # a size whose video (the upload staging beside the resident copy, and the synthesiser's tensor) does not fit is recorded as not measured BEFORE anything of it
        # is started; any error of a size that was started ends the script: nothing more is launched on a device that has reported one
        need = 3 * d1 * d2 * T * 4 + (8 << 30)
        free = torch.cuda.mem_get_info(0)[0] if torch.cuda.is_available() else None
        if free is not None and free < need:
            res["sizes"].append(dict(d1=d1, d2=d2, T=T, K=K, not_measured="needs %d bytes of device memory, %d are free" % (need, free)))
            continue
        eng = Engine(0)
        try:
            res["sizes"].append(run(eng, d1, d2, T, K, a.nb, 2))
        finally:
            eng.close()
    ring = os.path.join(ROOT, "profiles", "r06", "bench_c3_v9.json")
    if os.path.exists(ring):
        with open(ring) as fh:
            bench = json.load(fh)

        def find(node, key):                                   # the first per-kernel table of the bench line that names the kernel
            if isinstance(node, dict):
                if isinstance(node.get(key), (int, float)):
                    return float(node[key])
                node = list(node.values())
            if isinstance(node, list):
                for v in node:
                    got = find(v, key)
                    if got is not None:
                        return got
            return None
        res["ring_fit_512x512x10000_ms"] = dict(source="profiles/r06/bench_c3_v9.json", bg_ring_solve=find(bench, "bg_ring_solve"), bg_win_proj=find(bench, "bg_win_proj"))
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(res, fh, indent=1, sort_keys=True)
    print(json.dumps(res, indent=1, sort_keys=True))


if __name__ == "__main__":
    main()
