"""Fixtures of the initTemporal tests: seeded synth videos (cnmf_e_amd.synth's recipe with the footprints placed by hand).

Every case has TWO recordings of one field of view: the same footprints and background field, other traces, other noise.  W and b0 come from one oracle
background fit (cnmfe_oracle.fit_ring_model) of the first; initTemporal runs on the second.  Everything the engine takes as float32 (video, A, W, b0) is
rounded here, so the float64 oracle and the engine start from the same numbers.  The seeds were searched on the CPU so that the winner of every pixel of the
rough start (HALS_temporal.m:37) beats the runner-up by at least MARGIN relative: tests/test_init_temporal_oracle.py::test_fixture_margins asserts it."""
import functools

import numpy as np
import scipy.sparse as sp

import cnmfe_oracle as orc
import init_temporal_oracle as ito
from cnmf_e_amd import synth

MARGIN = 1e-6
DECONV = dict(smin=-5.0, optimize_pars=True, optimize_b=True, max_tau=100.0)        # the deconv_options of demo_large_data_1p.m:38-43

# name: (d1, d2, T, patch dims, ring radius, centres (0-based row, column), seed, deconvolution)
_GRID = [(20.0 + i, 20.0 + j) for j in range(9) for i in range(9)][:80]
CASES = {
    # 2 x 2 patches with halo; (8, 19.5) and (21.5, 8) sit on a patch border; the lower right block holds no footprint; T % 4 = 3
    "A": (44, 40, 403, [22, 20], 5, [(7.0, 7.0), (8.0, 19.5), (9.0, 30.0), (30.0, 6.0), (36.0, 9.0), (21.5, 8.0)], 11, False),
    "B": (40, 36, 600, [40, 36], 8, [(10.0, 9.0), (13.0, 14.0), (27.0, 24.0), (30.0, 10.0)], 12, True),
    "C": (40, 36, 300, [40, 36], 8, [(10.0, 9.0), (14.0, 13.0), (28.0, 25.0)], 13, False),
    # 80 footprints one pixel apart on one spot: (E - W)' At of all of them meets the same 16 x 16 blocks
    "D": (48, 48, 200, [48, 48], 5, _GRID, 14, False),
}


class Case:
    pass


def _recording(d1, d2, T, A, field, seed, noise=1.0):
    """synth.make_factors' traces and background time course + synth.make_video's sum, for given footprints and field"""
    rng = np.random.default_rng(seed)
    K = A.shape[1]
    spikes = (rng.random((K, T)) < 0.01) * rng.uniform(5.0, 15.0, (K, T))
    C = synth._ar1(spikes, 0.95)
    slow = synth._ar1(rng.normal(0.0, 1.0, T), 0.999) * np.sqrt(1 - 0.999 ** 2)
    bg_time = 1.0 + 0.1 * slow
    Y = C.T @ A.T.toarray() + np.outer(bg_time, field) + 1000.0 + noise * rng.normal(0.0, 1.0, (T, d1 * d2))
    return np.ascontiguousarray(Y.astype(np.float32)), C


@functools.lru_cache(maxsize=None)
def make(name, noise=1.0):
    """noise = 0: the second recording without its pixel noise (what the planted traces are recovered from)"""
    d1, d2, T, pdims, r, centres, seed, deconv = CASES[name]
    rng = np.random.default_rng(seed)
    amp = rng.uniform(0.5, 1.5, len(centres))
    A = synth._footprints(d1, d2, np.asarray(centres), amp, 1.5, 7).astype(np.float32)
    A.sort_indices()
    rr, cc = np.meshgrid(np.arange(d1), np.arange(d2), indexing="ij")
    field = np.zeros((d1, d2))
    for _ in range(8):
        r0, c0 = rng.uniform(0, d1), rng.uniform(0, d2)
        field += rng.uniform(100.0, 300.0) * np.exp(-((rr - r0) ** 2 + (cc - c0) ** 2) / (2 * (60.0 * max(d1, d2) / 512.0) ** 2))
    field = field.reshape(-1, order="F")
    Y1, C1 = _recording(d1, d2, T, A, field, seed * 1000 + 1)
    Y2, C2 = _recording(d1, d2, T, A, field, seed * 1000 + 2, noise)
    # the background of the first recording: one oracle fit per patch from the uniform ring (a first run)
    patch_pos, block_pos = orc.distribute_geometry(d1, d2, pdims, r)
    rs, cs = orc.get_nhood(r, None)
    A64 = sp.csc_matrix(A).astype(np.float64)
    W, b0 = {}, {}
    for n in range(patch_pos.shape[1]):
        for m in range(patch_pos.shape[0]):
            bp = ito.block_pixels(block_pos[m, n], d1)
            ip = orc.ind_patch_mask(patch_pos[m, n], block_pos[m, n])
            W0 = orc.build_ring_W(patch_pos[m, n], block_pos[m, n], d1, d2, rs, cs)
            A_b = A64[bp]
            ind = np.nonzero(np.asarray(A_b.sum(axis=0)).ravel() > 0)[0]
            Wf, b0f = orc.fit_ring_model(Y1[:, bp].T, A_b[:, ind] if ind.size else None, C1[ind] if ind.size else None, W0, np.nan, None, ip)
            Wf = sp.csr_matrix(Wf); Wf.sort_indices()
            W[(m, n)] = sp.csr_matrix((Wf.data.astype(np.float32), Wf.indices, Wf.indptr), shape=Wf.shape)
            b0[(m, n)] = np.asarray(b0f, dtype=np.float32)
    c = Case()
    c.name, c.d1, c.d2, c.T, c.pdims, c.r, c.K = name, d1, d2, T, pdims, r, len(centres)
    c.A, c.W, c.b0, c.Y, c.C_true, c.deconv = A, W, b0, Y2, C2, (dict(DECONV) if deconv else None)
    c.patch_pos, c.block_pos = patch_pos, block_pos
    return c


@functools.lru_cache(maxsize=None)
def reference(name):
    """the oracle's initTemporal of the case's second recording (computed once, shared, never modified)"""
    c = make(name)
    return ito.init_temporal(c.Y, c.A, c.W, c.d1, c.d2, c.pdims, c.r, c.deconv)
