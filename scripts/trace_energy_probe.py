"""Time of cnmfe_trace_energy at K = 500, T = 10000 on the bound matrix ("Temporal batches"): the call as the host sees it (it ends in a
synchronise) and its two kernels by device events.  Warm-up first, then 30000 timed calls (a window of about a second at ~33 us a call; `window_s` records it); median and range."""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main(out=None):
    from cnmf_e_amd.engine import Engine
    K, T, warm, reps = 500, 10000, 200, 30000                 # (30000 calls of ~33 us: a timed window of about a second)
    X = np.random.default_rng(0).standard_normal((K, T)).astype(np.float32)
    eng = Engine(0)
    try:
        eng.bind_traces(X)
        ref = (X.astype(np.float64) ** 2).sum(axis=1)
        e = eng.trace_energy(X)
        assert np.all(np.abs(e - ref) <= 2 * T * 2.0 ** -53 * ref)
        for _ in range(warm):
            eng.trace_energy(X)
        t = np.empty(reps)
        for i in range(reps):
            t0 = time.perf_counter()
            eng.trace_energy(X)
            t[i] = time.perf_counter() - t0
        eng.profile(True); eng.profile_reset()
        for _ in range(200):
            eng.trace_energy(X)
        tab = eng.profile_table()
        eng.profile(False)
        res = dict(K=K, T=T, bytes=K * T * 4, reps=reps, window_s=float(t.sum()),
                   call_us=dict(median=float(np.median(t) * 1e6), min=float(t.min() * 1e6), p90=float(np.quantile(t, 0.9) * 1e6)),
                   kernels_us={k: v["total_ms"] * 1e3 / v["calls"] for k, v in tab.items() if v["calls"] and k.startswith("trace_energy")})
        k_us = res["kernels_us"].get("trace_energy")
        if k_us:
            res["trace_energy_TBps"] = K * T * 4 / (k_us * 1e-6) / 1e12
    finally:
        eng.close()
    line = json.dumps(res)
    print(line)
    if out:
        with open(out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else None)
