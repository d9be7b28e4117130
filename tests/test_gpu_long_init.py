"""The peel session beyond the 20 416 frames a trace and its Welch transform share one workgroup's LDS (k_seed_stats_long, k_peel_trace_stats_long; the chunked
box kernels of csrc/peel.hpp at these lengths), against the float64 oracle tests/greedy_oracle.py on the fixture of tests/long_cases.py: 30 x 28 pixels, two
true neurons, gSig 2, gSiz 9, nk = 1, at 20 417 and 74 000 frames (tests/test_long_fixtures.py pins the fixture's margins on the CPU).

The oracle's accepted centres are forced as seeds.  After EACH extract: the sets {corr > 0.9} and {corr < 0.3} equal the oracle's; ci / max|ci| <= 2e-6 and
ai / max|ai| <= 3e-5 (the bounds of tests/test_gpu_init.py); norm_ci, max_diff, std_diff within 1e-6 relative; sn_ci within 2e-4 relative (the Welch estimator's
bound at these lengths, tests/test_gpu_edges.py::test_get_sn_of_long_recordings).  From the second extract on the videos carry the earlier applies' rank-1
subtractions, so the chunked kernels are exercised at these lengths.  Per-sample threshold decisions cannot equal the oracle's at this length (see
tests/test_gpu_long_seed.py): the zero patterns of the apply's boxes and the Cn box are NOT compared here (tests/test_gpu_long_flavour.py covers them bit for
bit against the LDS flavour); the PNR box is, relative 2e-4, on the entries non-zero in both, which must be at least half of the box.

End to end at 20 417 frames: initComponents_parallel, then initComponents_residual_parallel with the first pass's neurons.  The first pass returns the oracle's
centres; one lies within 2 pixels of each true centre, and its C row correlates above 0.9 with the true trace (the oracle's own rows: 0.994 and 0.989, pinned
on the CPU) and equals the oracle's correlation to 1e-6; the second pass runs and leaves A and C with equal K."""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import long_cases as lc

pytestmark = pytest.mark.gpu

CI_TOL, AI_TOL = 2e-6, 3e-5
STAT_TOL = 1e-6
PNR_TOL = 2e-4


def _options():
    from cnmf_e_amd.sources2d import Options
    p = lc.PEEL
    return Options(ring_radius=p["r"], gSig=p["gSig"], gSiz=p["gSiz"], nk=1, min_corr=p["min_corr"], min_pnr=p["min_pnr"], maxIter=3)


def _sources(eng, T):
    from cnmf_e_amd.sources2d import PatchedVideo, Sources2D
    f, Y = lc.peel_video(T)
    d1, d2 = lc.PEEL["dims"]
    video = PatchedVideo(d1, d2, T, [d1, d2], lc.PEEL["r"], eng)
    video.upload_from_full(Y)
    return f, Sources2D(video, _options(), f.A_init, f.C_init, f.sn)


def _maxrel(a, b):
    return float(np.max(np.abs(np.asarray(a) - np.asarray(b))) / np.max(np.abs(b)))


@pytest.mark.parametrize("T", [20417, 74000])
def test_steps_under_forced_seeds(T, observed):
    ora = lc.peel_oracle(T, forced=True)
    eng = lc.engine()
    try:
        f, s = _sources(eng, T)
        log = []
        s._init_observer = lambda idx, kind, data: log.append((kind, data))
        s.initComponents_parallel(seeds=[tuple(int(x) for x in rc) for rc in lc.PEEL_CENTRES[T]])
    finally:
        eng.close()
    steps = ora["blocks"][(0, 0)]["steps"]
    assert [k for k, _ in log] == [st["kind"] for st in steps]
    e = dict(ci=0.0, ai=0.0, stat=0.0, sn=0.0, pnr=0.0)
    nex = 0
    for (kind, d), o in zip(log, steps):
        assert (d["r"], d["c"]) == (o["r"], o["c"])
        if kind == "extract":
            nex += 1
            with np.errstate(invalid="ignore"):
                assert np.array_equal(d["corr"] > 0.9, o["hi"]) and np.array_equal(d["corr"] < 0.3, o["lo"]), (d["r"], d["c"])
            e["ci"] = max(e["ci"], _maxrel(d["ci"], o["ci"])); e["ai"] = max(e["ai"], _maxrel(d["ai"], o["ai"]))
            for k in ("norm_ci", "max_diff", "std_diff"):
                e["stat"] = max(e["stat"], abs(d["stats"][k] - o["stats"][k]) / abs(o["stats"][k]))
            e["sn"] = max(e["sn"], abs(d["stats"]["sn_ci"] - o["stats"]["sn_ci"]) / o["stats"]["sn_ci"])
        else:
            both = (d["pnr"] != 0) & (o["pnr"] != 0)
            assert both.mean() >= 0.5, both.mean()
            e["pnr"] = max(e["pnr"], float(np.max(np.abs(d["pnr"] - o["pnr"])[both] / o["pnr"][both])))
            assert np.all(np.isfinite(d["cn"])) and d["cn"].max() <= 1.0
    observed["long_init_steps_%d" % T] = e
    print("long init steps T = %d: %d extracts  ci %.3e  ai %.3e  norm / diff stats %.3e  sn_ci %.3e  PNR rel %.3e" % (T, nex, e["ci"], e["ai"], e["stat"], e["sn"], e["pnr"]))
    assert nex >= 2
    assert e["ci"] <= CI_TOL and e["ai"] <= AI_TOL, e
    assert e["stat"] <= STAT_TOL, e
    assert e["sn"] <= lc.SN_TOL, e
    assert e["pnr"] <= PNR_TOL, e


def test_end_to_end_two_passes():
    T = 20417
    ora = lc.peel_oracle(T, forced=False)
    eng = lc.engine()
    try:
        f, s = _sources(eng, T)
        center, Cn, PNR = s.initComponents_parallel()
        C1 = np.array(s.C, dtype=np.float64)
        K1 = s.A.shape[1]
        s.update_background_parallel()
        s.initComponents_residual_parallel()
        assert s.A.shape[1] == np.asarray(s.C).shape[0] >= K1 and np.all(np.isfinite(np.asarray(s.C)))
    finally:
        eng.close()
    assert np.array_equal(center, ora["center"]), (center, ora["center"])
    d1, d2 = lc.PEEL["dims"]
    for k in range(f.K):
        tr = np.unravel_index(int(np.argmax(f.A_true[:, k].toarray().ravel())), (d1, d2), order="F")
        dist = [max(abs(int(r) - 1 - tr[0]), abs(int(c) - 1 - tr[1])) for r, c in center]
        j = int(np.argmin(dist))
        assert dist[j] <= 2, (k, tr, center)
        got, ref = np.corrcoef(C1[j], f.C_true[k])[0, 1], np.corrcoef(ora["C"][j], f.C_true[k])[0, 1]
        print("long init end to end: true neuron %d, centre %s, corr(C, C_true) engine %.6f oracle %.6f" % (k, center[j].tolist(), got, ref))
        assert got > 0.9, got
        assert abs(got - ref) <= 1e-6, (got, ref)
