"""Times of the long flavours of the session and trace kernels (HIP events of the engine's profiler, Engine.profile): seed_stats on a 128 x 128 block,
peel_trace_stats of one extract on it, trace_tags and trace_diff_spikes for K = 500 traces, at 24 000 and 74 000 frames.  Nothing is compared: the parent of
the change that added these kernels refused the calls.  `python scripts/long_flavour_times.py [out.txt]`  (profiles/long_flavour/README.md)."""
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from cnmf_e_amd.engine import Engine
from cnmf_e_amd.sources2d import PatchedVideo

lines = []


def say(s):
    print(s, flush=True)
    lines.append(s)


def table(eng, names, tag):
    t = eng.profile_table()
    for n in names:
        if n in t:
            say("%-28s %-18s calls %3d   total %10.3f ms   per call %10.3f ms" % (tag, n, t[n]["calls"], t[n]["total_ms"], t[n]["total_ms"] / max(t[n]["calls"], 1)))


def main():
    d1 = d2 = 128
    K = 500
    for T in (24000, 74000):
        eng = Engine(0)
        try:
            rng = np.random.default_rng(T)
            t0 = time.time()
            Y = rng.standard_normal((T, d1 * d2), dtype=np.float32)
            Y[:, 64 * d1 + 64] += (rng.random(T) < 0.01) * 20.0                  # one pixel with events, the seed of the extract
            video = PatchedVideo(d1, d2, T, [d1, d2], 3, eng)
            video.upload_from_full(Y)
            del Y
            say("T = %d: 128 x 128 video made and uploaded in %.1f s" % (T, time.time() - t0))
            eng.seed_images(0, None)                                             # warm-up: allocations, first launch
            eng.profile(True); eng.profile_reset()
            eng.seed_images(0, None)
            table(eng, ["seed_stats", "seed_corr"], "seed_images 128x128 T=%d" % T)
            eng.peel_open(0, None)
            eng.peel_extract(0, 64, 64, 9)
            eng.profile_reset()
            eng.peel_extract(0, 64, 64, 9)
            table(eng, ["peel_trace_stats", "peel_traces", "peel_corr_part", "peel_mom_part"], "peel_extract gSiz 9 T=%d" % T)
            eng.peel_close(0)
            C = rng.standard_normal((K, T), dtype=np.float32)
            eng.traces_load(C, C + np.float32(0.1), np.maximum(C, 0))
            eng.trace_tags(); eng.trace_diff_spikes(C)
            eng.profile_reset()
            eng.trace_tags(); eng.trace_diff_spikes(C)
            table(eng, ["trace_tags", "trace_diff_spikes"], "K = %d T=%d" % (K, T))
        finally:
            eng.close()
    if len(sys.argv) > 1:
        with open(sys.argv[1], "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
