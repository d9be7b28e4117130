"""What a merge and a tag call cost: merge_high_corr and tag_neurons_parallel at K = 500, T = 10000 with the demo's thresholds (demo_large_data_1p.m:63:
merge_thr_spatial = [0.8, 0.4, -inf]; min_pnr = 3), on the engine -- the matrices resident, as after update_temporal_parallel with deconvolution -- and the same
methods of tests/merge_oracle.py (float64 NumPy, the literal form with `data`) on this machine's host.  Warm-up, then repetitions; median and spread of both.

    python scripts/merge_probe.py [--K 500] [--T 10000] [--pairs 5] [--reps 7] [--oracle-reps 3] [--out profiles/merge/probe.json]

The record is the figures, there is no pass mark.  The field of view is small (64 x 64: the merges do not read the video, only the engine's set-up does)."""
import argparse
import json
import os
import sys
import time

import numpy as np
import scipy.sparse as sp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p_ in (ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "oracle")):
    sys.path.insert(0, p_)


def build(K, T, pairs, seed=0, d1=64, d2=64):
    from cnmf_e_amd import synth
    rng = np.random.default_rng(seed)
    rr, cc = np.mgrid[0:d1, 0:d2]
    cols = []
    ctr = np.stack([rng.uniform(5, d1 - 6, K), rng.uniform(5, d2 - 6, K)], axis=1)
    for k in range(pairs):                                  # neuron K - 1 - k sits one pixel beside neuron k and shows the same activity
        ctr[K - 1 - k] = ctr[k] + (1.0, 0.0)
    for r, c in ctr:
        g = np.exp(-((rr - r) ** 2 + (cc - c) ** 2) / 8.0) * ((np.abs(rr - r) <= 4.5) & (np.abs(cc - c) <= 4.5))
        cols.append(sp.csc_matrix(g.ravel(order="F")[:, None]))
    A = sp.hstack(cols, format="csc").astype(np.float32)
    spikes = (rng.random((K, T)) < 0.01) * rng.uniform(5.0, 15.0, (K, T))
    R = synth._ar1(spikes, 0.95)
    for k in range(pairs):
        R[K - 1 - k] = R[k]
    R = (R + rng.normal(0.0, 0.3, (K, T)) + 0.7).astype(np.float32)
    return A, R, d1, d2


def stats(ts):
    ts = np.asarray(ts) * 1e3
    return dict(median_ms=float(np.median(ts)), min_ms=float(ts.min()), max_ms=float(ts.max()), n=int(ts.size))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--K", type=int, default=500); ap.add_argument("--T", type=int, default=10000); ap.add_argument("--pairs", type=int, default=5)
    ap.add_argument("--reps", type=int, default=7); ap.add_argument("--oracle-reps", type=int, default=3); ap.add_argument("--out", default=None)
    a = ap.parse_args()
    from cnmf_e_amd.engine import Engine
    from cnmf_e_amd.sources2d import PatchedVideo, Sources2D, Options
    import merge_oracle as mo
    thr, min_pnr = [0.8, 0.4, -np.inf], 3.0
    A, R, d1, d2 = build(a.K, a.T, a.pairs)
    eng = Engine(0)
    video = PatchedVideo(d1, d2, a.T, [d1, d2], 6, eng)
    video.upload_from_full(np.zeros((a.T, d1 * d2), dtype=np.float32))
    s = Sources2D(video, Options(ring_radius=6, deconv_flag=True), A, R, np.ones(d1 * d2, dtype=np.float32))
    s.C_raw = s.C                                           # the stitched C_raw as the bound matrix: deconvTemporal runs where it lies and leaves C, C_raw, S resident
    s.deconvTemporal()
    state = dict(A=s.A, C=np.array(s.C), C_raw=np.array(s.C_raw), S=np.array(s.S), kp=np.array(s.P["kernel_pars"]))
    n0 = eng.counter("merge_trace_uploads")
    t_tag, t_merge, merged = [], [], None
    for i in range(a.reps + 1):                             # (the first round is the warm-up)
        eng.synchronize(); t0 = time.perf_counter(); tags = s.tag_neurons_parallel(min_pnr); t1 = time.perf_counter()
        merged, _ = s.merge_high_corr(False, thr); eng.synchronize(); t2 = time.perf_counter()
        if i:
            t_tag.append(t1 - t0); t_merge.append(t2 - t1)
        uploads = eng.counter("merge_trace_uploads") - n0
        # back to the state before the merge, resident again (not timed; these uploads are the probe's, not the method's)
        s.A, s.C, s.C_raw, s.S = state["A"], state["C"], state["C_raw"], state["S"]; s.P["kernel_pars"] = state["kp"]
        eng.traces_load(s.C, s.C_raw, s.S, state["kp"])
        n0 = eng.counter("merge_trace_uploads")
    eng.close()
    o_tag, o_merge, o_merged = [], [], None
    for i in range(a.oracle_reps + 1):
        t0 = time.perf_counter(); otags, _ = mo.tag_neurons(state["A"], state["C"], state["C_raw"], state["S"], 5.0, True, min_pnr); t1 = time.perf_counter()
        res = mo.merge_high_corr(state["A"], state["C"], state["C_raw"], state["S"], state["kp"], thr); t2 = time.perf_counter()
        o_merged = res["merged_ROIs"]
        if i:
            o_tag.append(t1 - t0); o_merge.append(t2 - t1)
    out = dict(K=a.K, T=a.T, merge_thr=[0.8, 0.4, "-inf"], min_pnr=min_pnr, groups_merged=len(merged), groups_equal_oracle=[g.tolist() for g in merged] == [g.tolist() for g in o_merged],
               tags_equal_oracle=bool(np.array_equal(tags, otags)), uploads_in_the_timed_calls=int(uploads), host_threads=os.environ.get("OMP_NUM_THREADS"),
               engine=dict(merge_high_corr=stats(t_merge), tag_neurons_parallel=stats(t_tag)), host_oracle=dict(merge_high_corr=stats(o_merge), tag_neurons_parallel=stats(o_tag)))
    line = json.dumps(out)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
