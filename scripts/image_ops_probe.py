"""Host path against device path of the image operations on single footprints, in one session.

    python scripts/image_ops_probe.py [--out profiles/image_ops/probe.json] [--sizes 512x512x500,256x256x100]

Per size (d1 x d2 x K, synthetic footprints from cnmf_e_amd.synth, search_method = 'dilate' with strel('disk', 4, 0), spatial_constraints.circular) it times, with
image_ops_on_device False (cnmf_e_amd.hostops, the path before the kernels existed) and True (csrc/footprint_ops.hpp):
    search      Sources2D._search_location_csc()            the 'dilate' masks of one spatial update
    circular    the circular tail of _spatial_finish        circular_constraints of every column of A
    compact     Sources2D.compactSpatial()
    spatial     Sources2D.update_spatial_parallel()         the whole update, both of the above inside
Each figure is the median wall time of --runs calls (default 10) after --warmup calls (default 2), the engine synchronised before the clock is read; min and max
are kept beside it.  A host-path call that takes longer than --slow seconds is run --slow-runs times after one warm-up instead (the JSON says which): at 512 x 512
the host masks are K passes over a quarter of a million pixels each.  One JSON document on stdout and in --out."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def timed(fn, sync, runs, warmup, slow, slow_runs, pre=None, post=None):
    """pre / post: what runs around every call outside the clock"""
    def once():
        if pre:
            pre()
        sync()
        t0 = time.perf_counter(); fn(); sync()
        dt = time.perf_counter() - t0
        if post:
            post()
        return dt
    first = once()
    if first > slow:
        runs, warmup = slow_runs, 0                                       # (the call above was the warm-up)
    else:
        warmup = max(warmup - 1, 0)
    for _ in range(warmup):
        once()
    ts = np.asarray([once() for _ in range(runs)]) * 1e3
    return dict(median_ms=float(np.median(ts)), min_ms=float(ts.min()), max_ms=float(ts.max()), runs=int(runs), first_call_ms=first * 1e3)


def probe(d1, d2, K, T, a):
    from cnmf_e_amd import synth
    from cnmf_e_amd.engine import Engine
    from cnmf_e_amd.sources2d import PatchedVideo, Sources2D, Options
    f = synth.make_factors(d1, d2, T, K, 11)
    Y = synth.make_video(f, np.float32)
    eng = Engine(0)
    try:
        video = PatchedVideo(d1, d2, T, [d1, d2], 15, eng)
        video.upload_from_full(Y)
        del Y
        s = Sources2D(video, Options(ring_radius=15, spatial_algorithm="hals", maxIter=5, search_method="dilate",
                                     spatial_constraints={"circular": True, "connected": True}), f.A_init, f.C_init, f.sn)
        s.update_background_parallel()
        A0 = s.A
        out = dict(d1=d1, d2=d2, K=K, T=T, nnz=int(A0.nnz))

        def search():
            s.options.se = "disk4"
            s._search_location_csc()

        def circular():
            s._circular_columns(A0)

        def compact():
            s.A = A0
            s.compactSpatial()

        def spatial():                                                      # (inside a whole iteration: the background before it and the temporal update after it are not timed)
            s.update_spatial_parallel()

        def before_spatial():
            s.options.se = "disk4"
            s.update_background_parallel()

        for name, fn in (("search", search), ("circular", circular), ("compact", compact), ("spatial", spatial)):
            for on in (False, True):
                s.image_ops_on_device = on
                around = dict(pre=before_spatial, post=s.update_temporal_parallel) if name == "spatial" else {}
                r = timed(fn, eng.synchronize, a.runs, a.warmup, a.slow, a.slow_runs, **around)
                if on:
                    r["host_columns"] = int(eng.counter("image_ops_host_columns"))
                out.setdefault(name, {})["device" if on else "host"] = r
                print("%4dx%-4d K=%-4d %-9s %-6s median %10.2f ms  (min %.2f, max %.2f, %d runs)" % (d1, d2, K, name, "device" if on else "host", r["median_ms"],
                                                                                                     r["min_ms"], r["max_ms"], r["runs"]), file=sys.stderr, flush=True)
            out[name]["speedup"] = out[name]["host"]["median_ms"] / out[name]["device"]["median_ms"]
        return out
    finally:
        eng.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "image_ops", "probe.json"))
    ap.add_argument("--sizes", default="512x512x500,256x256x100")
    ap.add_argument("--frames", type=int, default=256)
    ap.add_argument("--runs", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--slow", type=float, default=2.0)
    ap.add_argument("--slow-runs", type=int, default=3)
    a = ap.parse_args()
    doc = dict(what="image operations on single footprints: hostops against the engine, median wall ms per call", sizes=[])
    for sz in a.sizes.split(","):
        d1, d2, K = (int(x) for x in sz.split("x"))
        doc["sizes"].append(probe(d1, d2, K, a.frames, a))
    txt = json.dumps(doc, indent=1, sort_keys=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        fh.write(txt + "\n")
    print(txt)


if __name__ == "__main__":
    main()
