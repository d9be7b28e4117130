"""Fixtures of initTemporal under background_model = 'svd': small deterministic recordings of a 40 x 36 field of view cut into 2 x 2 patches of uneven size
(22 + 18 rows, 20 + 16 columns) with a halo of 3 pixels, T = 203 frames (not a multiple of 4).

Every case has TWO recordings of one field of view, as tests/init_temporal_cases.py: the same footprints and the same `nb` background maps (the smooth maps of
tests/svd_bg_cases.py, strengths a factor 3 apart, a baseline of 200, white noise of 0.5), other traces, other background time courses, other noise.  The spatial
background b of every patch comes from the oracle's fit of the FIRST recording (svd_bg_oracle.fit_svd_model); each column is then scaled to a Euclidean norm of 3
on its patch, the scale of a footprint.  (The fit's own scale u * s puts 1e8 between the diagonal entries of [A, b]'[A, b]; the engine's Cholesky does not mind, but
the conditions the CPU tests assert on these inputs -- cond(G) <= 1e4 -- are about the conditioning of the PROBLEM, not of its units.)  initTemporal runs on the
SECOND recording.  Everything the engine takes as float32 (video, A) is rounded here; b is float64 on both sides.

    a   nb 1, 5 neurons, two of them straddling a patch border
    b   nb 3, 21 neurons (n = 24 over the field); the upper left patch holds fifteen of them: n = 18 there, past one 16-tile and off a multiple of 16
    c   nb 8, 80 neurons one pixel apart (init_temporal_cases._GRID, moved into the lower right patch, which holds all of every footprint: a footprint that only
        reaches into a patch with its tail is collinear with its neighbours' tails there): n = 88 -- six 16-tiles of the solve -- and the first 16 x 16 block of that
        patch meets 88 columns: two projection passes.  Narrow footprints (sigma 0.6): one pixel apart, wider ones are collinear.  The other patches are empty
    d   nb 0: A'A \\ A'Yc alone
    e   nb 2, the second column of b all zero in every patch
    f   nb 1, the lower right patch without a neuron
"""
import functools

import numpy as np
import scipy.sparse as sp

import init_temporal_cases as itc
import svd_bg_cases as sc
import svd_bg_oracle as so
import svd_init_temporal_oracle as sio
from cnmf_e_amd import synth

D1, D2, T, PDIMS, HALO = 40, 36, 203, [22, 20], 3
B_NORM = 3.0
DECONV = dict(itc.DECONV)

_C5 = [(8.3, 7.1), (21.4, 9.2), (9.6, 19.7), (30.2, 8.4), (29.1, 27.3)]                   # (21.4, 9.2): the row border, (9.6, 19.7): the column border
_C21 = ([(3.2 + 4.4 * i, 3.3 + 4.1 * j) for i in range(5) for j in range(3)]               # fifteen in the upper left patch: n = 18 there
        + [(30.3, 8.1), (33.1, 27.2), (9.2, 27.4), (15.3, 31.2), (27.4, 18.9), (5.1, 24.3)])
_C80 = [(r + 5.0, c + 3.0) for r, c in itc._GRID]                                          # rows 25 .. 33, columns 23 .. 31: inside the lower right patch with their 7 x 7 boxes
_CF = [(8.3, 7.1), (21.4, 9.2), (9.6, 19.7), (30.2, 8.4), (11.0, 28.5)]                    # nothing in rows >= 22, columns >= 20
# name: (nb, centres, footprint sigma, zero columns of b, seed)
CASES = {
    "a": (1, _C5, 1.5, (), 31),
    "b": (3, _C21, 1.2, (), 32),
    "c": (8, _C80, 0.6, (), 33),
    "d": (0, _C5, 1.5, (), 34),
    "e": (2, _C5, 1.5, (1,), 35),
    "f": (1, _CF, 1.5, (), 36),
}


class Case:
    pass


def _maps(nb):
    rr, cc = np.meshgrid((np.arange(D1) + 0.5) / D1, (np.arange(D2) + 0.5) / D2, indexing="ij")
    out = []
    for i in range(nb):
        m = np.cos(np.pi * (i + 1) * rr) * np.cos(np.pi * ((i + 1) // 2) * cc) + 0.3 * np.sin(np.pi * (i + 2) * cc)      # svd_bg_cases.make_case
        out.append((m / np.sqrt(np.mean(m * m))).reshape(-1, order="F"))
    return np.asarray(out).reshape(nb, D1 * D2)


def _recording(A, maps, seed, T=T, rate=0.02):
    rng = np.random.default_rng(seed)
    K, nb = A.shape[1], maps.shape[0]
    spikes = (rng.random((K, T)) < rate) * rng.uniform(5.0, 12.0, (K, T))
    C = synth._ar1(spikes, 0.9)
    g = np.zeros((nb, T))
    for i in range(nb):
        x = synth._ar1(rng.normal(0.0, 1.0, T), 0.97)
        g[i] = (60.0 / 3.0 ** i) * (x - x.mean()) / x.std()
    Y = C.T @ A.T.toarray() + g.T @ maps + sc.BASE + rng.normal(0.0, sc.NOISE, (T, D1 * D2))
    return np.ascontiguousarray(Y, dtype=np.float32), C, g


@functools.lru_cache(maxsize=None)
def make(name):
    nb, centres, sig, zero_cols, seed = CASES[name]
    rng = np.random.default_rng(seed)
    A = synth._footprints(D1, D2, np.asarray(centres), rng.uniform(0.8, 1.2, len(centres)), sig, 7).astype(np.float32)
    A.sort_indices()
    nfit = nb - len(zero_cols)
    maps = _maps(nfit)
    Y1, C1, _ = _recording(A, maps, seed * 1000 + 1)
    Y2, C2, g2 = _recording(A, maps, seed * 1000 + 2)
    patch_pos, block_pos = sio.orc.distribute_geometry(D1, D2, PDIMS, HALO)
    A64 = sp.csc_matrix(A).astype(np.float64)
    b = {}
    for n in range(patch_pos.shape[1]):
        for m in range(patch_pos.shape[0]):
            bp = sio.ito.block_pixels(block_pos[m, n], D1)
            ip = sio.orc.ind_patch_mask(patch_pos[m, n], block_pos[m, n])
            A_b = A64[bp]
            ind = np.nonzero(np.asarray(A_b.sum(axis=0)).ravel() > 0)[0]
            bf = so.fit_svd_model(Y1[:, bp].T.astype(np.float64), nfit, A_b[:, ind] if ind.size else None, C1[ind] if ind.size else None, ind_patch=ip)[0]
            bm = np.zeros((int(ip.sum()), nb))
            live = [i for i in range(nb) if i not in zero_cols]
            bm[:, live] = bf * (B_NORM / np.sqrt((bf ** 2).sum(axis=0)))[None, :] if nfit else bf
            b[(m, n)] = bm
    c = Case()
    c.name, c.d1, c.d2, c.T, c.pdims, c.halo, c.K, c.nb = name, D1, D2, T, PDIMS, HALO, len(centres), nb
    c.A, c.Y, c.b, c.C_true, c.g_true, c.zero_cols = A, Y2, b, C2, g2, zero_cols
    c.patch_pos, c.block_pos = patch_pos, block_pos
    return c


@functools.lru_cache(maxsize=None)
def reference(name, deconv=False):
    """the oracle's initTemporal of the case's second recording (computed once, shared, never modified)"""
    c = make(name)
    return sio.init_temporal(c.Y, c.A, c.b, c.d1, c.d2, c.pdims, c.halo, dict(DECONV) if deconv else None)


@functools.lru_cache(maxsize=None)
def batch_recording(frames=(96, 80), nb=1, seed=41):
    """one recording of the field cut into temporal batches (tests/test_gpu_svd_batch.py): case a's footprints, a spike every twenty frames so that a batch of 96
    frames shows every neuron.  Returns (Y (sum(frames), d) float32, the true A, the frame ranges [(t0, t1)])"""
    rng = np.random.default_rng(seed)
    A = synth._footprints(D1, D2, np.asarray(_C5), rng.uniform(0.8, 1.2, len(_C5)), 1.5, 7).astype(np.float32)
    A.sort_indices()
    Y, _, _ = _recording(A, _maps(nb), seed * 1000, T=int(sum(frames)), rate=0.05)
    edges = np.concatenate([[0], np.cumsum(frames)])
    return Y, A, [(int(edges[i]), int(edges[i + 1])) for i in range(len(frames))]
