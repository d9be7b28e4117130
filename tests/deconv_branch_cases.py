"""Inputs of the deconvolution branch tests (numpy only, no engine): named case families for k_deconv's option branches, trace edges and pool sizes.

A case is (name, Y float32 [K, T], opts dict, tags): the traces of one (T, opts) stacked into one matrix, so a case is ONE deconv_temporal call; tags[k]
names the branch row k is there to reach.  tests/test_deconv_branch_cases.py asserts on the oracle alone that every row reaches its branch and is
well-conditioned (the oracle rerun with sn * (1 +- 1e-6) keeps the spike support and moves g and C by < 1e-5), which is what lets
tests/test_gpu_deconv_branches.py demand identical spike support of the engine.  A row that fails that check is RESEEDED here (the seed tables below), never
skipped: there is no exclusion list, and the host test asserts the table's size.

Branch tags:
  restart        first estimate > gmax under optimize_b: foopsi_oasisAR1.m:104-108 re-estimates g and stops (pars == the first estimate again)
  update_g       optimize_b = false, first estimate > gmax: :82-90 knows no gmax test, update_g runs (pars != the first estimate)
  plain          the option row itself is the branch (no b, no update_g, a fixed smin, non-negativity alone, the iteration cap)
  pools          pool lengths at and beside 1, 2, 3 tasks of DTK = 31 samples, runs longer than a wave, events denser than six samples
  rule015        raw AR(1) estimate negative: estimate_time_constant.m:64 -> g = 0.15
  giveup         raw estimate beyond +-1: deconvolveCa.m:84-89 gives up, pars = 0, C = C_raw, S = 0
  nan            a NaN in the row: deconvTemporal.m:37-40, C = S = C_raw = 0
  ties           >= 10 samples equal to the 15 % order statistic (and to its upper neighbour)"""
import functools

import numpy as np

DTK = 31                                    # samples per task in k_deconv (csrc/deconv.hip)
DEMO = dict(smin=-5.0, optimize_pars=True, optimize_b=True, max_tau=100.0)      # demo_large_data_1p.m:38-43
GMAX5 = float(np.exp(-1.0 / 5.0))           # max_tau = 5: 0.8187


def ar1_trace(T, seed, g=0.95, sn=0.3, rate=0.01, amp=1.5):
    """one trace of test_gpu_edges._ar1_traces (its K = 1 draw order)"""
    rng = np.random.default_rng(seed)
    s = (rng.random(T) < rate) * amp
    c = np.zeros(T)
    for t in range(T):
        c[t] = (g * c[t - 1] if t else 0.0) + s[t]
    return (c + 0.5 + sn * rng.standard_normal(T)).astype(np.float32)


# ---- options: every option row on the same traces -------------------------------------------------------------------------------------------------------
# lengths: even and odd order statistics, an unpaired last Welch segment, nfft = 256 with heavy zero padding, i + j >= T run-off at different lanes
OPTION_T = (64, 65, 127, 129, 257, 600)
OPTION_ROWS = (
    ("tau5", dict(max_tau=5.0), "restart"),
    ("tau5_nob", dict(max_tau=5.0, optimize_b=False), "update_g"),
    ("nob", dict(optimize_b=False), "plain"),
    ("nog", dict(optimize_pars=False, optimize_b=True), "plain"),
    ("smin06", dict(smin=0.6), "plain"),
    ("smin0", dict(smin=0.0), "plain"),
    ("maxiter1", dict(maxIter=1), "plain"),
    ("maxiter3", dict(maxIter=3), "plain"),
)
# per-trace seeds, searched on the CPU (scan upwards from 100 T): first estimate > GMAX5, and all eight option rows well-conditioned
OPTION_SEEDS = {
    64: (6400, 6403, 6405, 6406),
    65: (6500, 6501, 6502, 6503),
    127: (12700, 12701, 12702, 12703),
    129: (12900, 12902, 12903, 12904),
    257: (25700, 25701, 25702, 25703),
    600: (60000, 60001, 60002, 60003),
}


def option_traces(T):
    return np.stack([ar1_trace(T, s, rate=0.03 if T < 300 else 0.01) for s in OPTION_SEEDS[T]])


def options_cases():
    for T in OPTION_T:
        Y = option_traces(T)
        for rname, o, tag in OPTION_ROWS:
            opts = dict(DEMO); opts.update(o)
            yield ("options_T%d_%s" % (T, rname), Y, opts, [tag] * Y.shape[0])


# ---- pool_lengths: a spike of amplitude 1.5 every P frames ----------------------------------------------------------------------------------------------
POOL_P = (2, 3, 5, 7, 30, 31, 32, 62, 63, 64, 65, 93, 130)
POOL_T = (193, 520)
POOL_G, POOL_SN, POOL_SEED = 0.7, 0.05, 7          # (g = 0.7: the 5 sn threshold resolves every event down to P = 2, and the pools are exactly P long)


def pool_traces(T):
    rng = np.random.default_rng(POOL_SEED + T)
    Y = np.zeros((len(POOL_P), T), np.float32)
    for k, P in enumerate(POOL_P):
        c = np.zeros(T)
        for t in range(T):
            c[t] = (POOL_G * c[t - 1] if t else 0.0) + (1.5 if t % P == 0 else 0.0)
        Y[k] = c + POOL_SN * rng.standard_normal(T)
    return Y


def pool_cases():
    for T in POOL_T:
        yield ("pools_T%d" % T, pool_traces(T), dict(DEMO), ["pools"] * len(POOL_P))


# ---- time_constant: the 0.15 rule, the give-up path, the NaN guard --------------------------------------------------------------------------------------
WHITE_SEEDS = {96: (6, 9, 10, 13), 400: (3, 4, 20, 24)}        # raw estimate in (-0.9, -0.05)
PERIOD2_T = (64, 96, 401)
PERIOD2_SEEDS = (0, 1, 2, 3)                                   # raw estimate in (-1.03, -1.003)


def white_trace(T, seed):
    return (np.random.default_rng(seed).standard_normal(T) + 1).astype(np.float32)


def period2_trace(T, seed):
    return (2.0 + np.where(np.arange(T) % 2, -1.0, 1.0) + 0.3 * np.random.default_rng(seed).standard_normal(T)).astype(np.float32)


def time_constant_cases():
    for T, seeds in WHITE_SEEDS.items():
        yield ("white_T%d" % T, np.stack([white_trace(T, s) for s in seeds]), dict(DEMO), ["rule015"] * len(seeds))
    for T in PERIOD2_T:
        Y = np.stack([period2_trace(T, s) for s in PERIOD2_SEEDS])
        tags = ["giveup"] * len(PERIOD2_SEEDS)
        if T == 96:                                            # the NaN row rides between ordinary ones: its neighbours must come out untouched
            bad = ar1_trace(T, 5, rate=0.03); bad[41] = np.nan
            Y = np.vstack([Y[:2], bad[None], Y[2:], ar1_trace(T, 6, rate=0.03)[None]])
            tags = ["giveup", "giveup", "nan", "giveup", "giveup", "plain"]
        yield ("period2_T%d" % T, Y, dict(DEMO), tags)


# ---- ties: the options traces floored at 0.25 and rounded to quarter steps ------------------------------------------------------------------------------
def quantise(y):
    return (np.round(np.maximum(np.asarray(y, np.float64), 0.25) * 4) / 4).astype(np.float32)


def q15_pair(y):
    """the order statistics foopsi_oasisAR1.m:93 interpolates between (0-based rank floor(0.15 T - 0.5) and the next) and how often each value occurs"""
    s = np.sort(np.asarray(y, np.float64)); i = int(np.floor(0.15 * s.size - 0.5))
    return s[i], s[i + 1], int((s == s[i]).sum()), int((s == s[i + 1]).sum())


TIES_SEEDS = {64: (12800, 12801), 65: (13000, 13001), 127: (25401, 25402), 129: (25800, 25801), 257: (51400, 51401), 600: (120000, 120001)}   # searched alike, from 200 T


def straddle_trace(T, seed):
    """quarter steps with EXACTLY rank + 1 samples on the floor, shifted by -0.375: the quantile pair is (-0.125, +0.125), either value many times"""
    y = quantise(ar1_trace(T, seed, rate=0.03 if T < 300 else 0.01)).astype(np.float64)
    want = int(np.floor(0.15 * T - 0.5)) + 1
    lo, nxt = np.nonzero(y == 0.25)[0], np.nonzero(y == 0.5)[0]
    if lo.size > want:
        y[lo[want:]] = 0.5
    else:
        y[nxt[:want - lo.size]] = 0.25
    return (y - 0.375).astype(np.float32)


def ties_cases():
    for T in OPTION_T:
        rows = [quantise(ar1_trace(T, s, rate=0.03 if T < 300 else 0.01)) for s in TIES_SEEDS[T]]
        tags = ["ties"] * len(rows)
        if T == 257:
            rows.append(rows[0] - np.float32(10.0)); tags.append("ties_negative")      # all values negative: the complemented keys of fkey
            rows.append(straddle_trace(T, TIES_SEEDS[T][1])); tags.append("ties_straddle")
        yield ("ties_T%d" % T, np.stack(rows), dict(DEMO), tags)


# ---- hals: one small field of view through the fused sweep ----------------------------------------------------------------------------------------------
HALS = dict(d1=40, d2=36, K=4, T=300, r=5, seed=3, sweeps=2, opts=dict(DEMO, max_tau=5.0))


@functools.lru_cache(maxsize=None)
def all_cases():
    return tuple(list(options_cases()) + list(pool_cases()) + list(time_constant_cases()) + list(ties_cases()))


N_CASES = 6 * 8 + 2 + 5 + 6                 # 61 calls
N_ROWS = 6 * 8 * 4 + 2 * 13 + (8 + 12 + 2) + (12 + 2)      # 254 traces


@functools.lru_cache(maxsize=None)
def reference(name):
    """the oracle's deconvTemporal of a case (computed once, shared, never modified): (C, C_raw, S, kernel_pars, sn)"""
    import oasis_oracle as oo
    for n, Y, opts, tags in all_cases():
        if n == name:
            out = oo.deconvTemporal(Y.astype(np.float64), **opts)
            for a in out:
                a.setflags(write=False)
            return out
    raise KeyError(name)
