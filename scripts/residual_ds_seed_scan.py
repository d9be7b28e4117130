"""Scan synthetic seeds for the fixtures of tests/residual_ds_cases.py, the DOWN-SAMPLED second pass (CPU only, the float64 oracle alone; the twin of
scripts/residual_seed_scan.py).

    python scripts/residual_ds_seed_scan.py CASE [first [count [workers]]]

For every seed the case's video is synthesised, the oracle fits the background once and runs the second pass on dsData of its own residual with the case's ssub / tsub
(OracleSources2D.init_residual -> ds_oracle.greedy_block_ds; automatic search, then the forced-seed run of the
accepted centres) on its own residual.  A seed is a CANDIDATE when both runs find at least two neurons, the forced run accepts the same centres, and every decision
margin clears FACTOR x the bounds of tests/greedy_cases.py (FACTOR = 2 here: the GPU test repeats the margin check on the residual the device exports, which
differs from the oracle's by fp32 rounding, and asks for half the bounds).  All candidates of the range are listed, tightest margin last, so that a fixture that
fails the device-side margin check can move to the next one."""
import os
import sys
from multiprocessing import Pool

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p_ in (ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "oracle")):
    sys.path.insert(0, p_)

FACTOR = 2.0


def one(args):
    import numpy as np
    import residual_ds_cases as rc
    name, seed = args
    c = dict(rc.CASES[name], seed=seed)
    try:
        o = rc.oracle_object(name, c)
        auto = rc.collect(c, o, o.init_residual)
        if auto["center"].shape[0] < 2:
            return seed, None, "K = %d" % auto["center"].shape[0]
        bad = rc.margins_clear(auto["margins"], FACTOR)
        if bad:
            return seed, None, "auto %s" % {k: "%.1e" % v for k, v in bad.items()}
        forced = rc.collect(c, o, o.init_residual, [tuple(int(x) for x in r) for r in auto["center"]])
        if not np.array_equal(forced["center"], auto["center"]):
            return seed, None, "forced run accepts other centres"
        bad = rc.margins_clear(forced["margins"], FACTOR)
        if bad:
            return seed, None, "forced %s" % {k: "%.1e" % v for k, v in bad.items()}
        import greedy_cases as gc
        worst = min(min(v / gc.MARGIN_MIN.get(k, gc.MARGIN_DEFAULT) for k, v in m.items()) for m in (auto["margins"], forced["margins"]))
        return seed, worst, "K = %d" % auto["center"].shape[0]
    except Exception as e:                                   # (a degenerate synthetic video: not a candidate)
        return seed, None, "%s: %s" % (type(e).__name__, e)


def main():
    name = sys.argv[1]
    first = int(sys.argv[2]) if len(sys.argv) > 2 else 0
    count = int(sys.argv[3]) if len(sys.argv) > 3 else 60
    workers = int(sys.argv[4]) if len(sys.argv) > 4 else 8
    good = []
    with Pool(workers) as pool:
        for seed, worst, why in pool.imap_unordered(one, [(name, s) for s in range(first, first + count)]):
            print("seed %4d  %s  %s" % (seed, "CANDIDATE x%.1f" % worst if worst is not None else "-", why), flush=True)
            if worst is not None:
                good.append((worst, seed))
    print("candidates (margin / bound, seed), widest first:", sorted(good, reverse=True))


if __name__ == "__main__":
    main()
