"""The float64 restatement of initTemporal under background_model = 'svd' (tests/svd_init_temporal_oracle.py) and the fixtures the GPU tests run it on
(tests/svd_init_temporal_cases.py).  The assertions on the fixtures are CONDITIONS ON THE INPUTS -- they make the reference's answer well defined to the digits
the GPU tests compare -- not measurements of any implementation."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import init_temporal_cases as itc
import svd_init_temporal_cases as sic
import svd_init_temporal_oracle as sio

NAMES = sorted(sic.CASES)


def test_oracle_recovers_planted_f_and_traces():
    """case a: in every patch with neurons the fitted f is the planted background time course (up to the scale and sign b carries) and the traces are the planted
    ones; b0 is the pixel mean"""
    c = sic.make("a")
    ref = sic.reference("a")
    assert len(ref["per_patch"]) == 4
    for idx, res in ref["per_patch"].items():
        assert res["f"].shape == (1, c.T)
        assert abs(np.corrcoef(res["f"][0], c.g_true[0])[0, 1]) > 0.999, idx
        pp = sio.ito.block_pixels(c.patch_pos[idx], c.d1)
        assert np.array_equal(res["b0"], c.Y[:, pp].astype(np.float64).T.mean(axis=1))
        # Ysig = Y - (b f + b0) is what the sweeps saw: no background is left in it beyond the noise
        assert np.abs(res["Ysig"]).mean() < 2.0
    for k in range(c.K):
        assert np.corrcoef(ref["C_raw"][k], c.C_true[k])[0, 1] > 0.95, k
    assert ref["C"] is ref["C_raw"]


def test_oracle_is_the_normal_equations_solution():
    """the start of the sweeps minimises |Yc - A C - b f| over (C, f) jointly: the gradient vanishes, and least squares on [A, b] gives the same numbers"""
    c = sic.make("b")
    idx = (0, 0)
    res = sic.reference("b")["per_patch"][idx]
    pp = sio.ito.block_pixels(c.patch_pos[idx], c.d1)
    ind = sic.reference("b")["ind"][idx]
    Y = c.Y[:, pp].astype(np.float64).T
    A = c.A.toarray().astype(np.float64)[pp][:, ind]
    M = np.hstack([A, c.b[idx]])
    X = np.linalg.lstsq(M, Y - Y.mean(axis=1, keepdims=True), rcond=None)[0]
    assert np.allclose(X[:ind.size], res["C0"], rtol=0, atol=1e-9 * np.abs(X).max())
    assert np.allclose(X[ind.size:], res["f"], rtol=0, atol=1e-9 * np.abs(X).max())


def test_zero_column_of_b_is_left_out():
    c = sic.make("e")
    ref = sic.reference("e")
    for idx, res in ref["per_patch"].items():
        assert not c.b[idx][:, 1].any() and c.b[idx][:, 0].any()
        assert res["f"].shape == (2, c.T) and not res["f"][1].any() and res["f"][0].any()
        assert np.isfinite(res["C_raw"]).all()
        assert res["G"].shape[0] == ref["ind"][idx].size + 1


def test_patch_without_neurons_is_skipped():
    ref = sic.reference("f")
    assert ref["ind"][(1, 1)].size == 0 and (1, 1) not in ref["per_patch"] and ref["f"][(1, 1)] is None and ref["b0"][(1, 1)] is None
    assert all(ref["ind"][idx].size for idx in [(0, 0), (1, 0), (0, 1)])


def test_case_shapes():
    """what the cases are there for: straddling neurons in a, n off a multiple of 16 in b, n > 64 and more than 64 columns over one 16 x 16 block in c, nb = 0 in d"""
    a = sic.reference("a")["ind"]
    assert sum(1 for k in range(5) if sum(k in ind for ind in a.values()) >= 2) >= 2
    nb_ = [ind.size + 3 for ind in sic.reference("b")["ind"].values()]
    assert max(nb_) > 16 and all(n % 16 for n in nb_)
    c = sic.reference("c")["ind"]
    assert c[(1, 1)].size + 8 > 64
    cc = sic.make("c")
    # the first 16 x 16 tile of the lower right BLOCK (rows 19 .., columns 17 .. of the field) holds a pixel of every footprint of that patch
    r0, c0 = cc.block_pos[1, 1][0] - 1, cc.block_pos[1, 1][2] - 1
    A = cc.A.tocsc()
    for k in c[(1, 1)]:
        rows = A.indices[A.indptr[k]:A.indptr[k + 1]]
        r, col = rows % cc.d1, rows // cc.d1
        assert np.any((r >= max(r0, 22)) & (r < r0 + 16) & (col >= max(c0, 20)) & (col < c0 + 16)), k
    assert sic.make("d").nb == 0 and all(b.shape[1] == 0 for b in sic.make("d").b.values())


@pytest.mark.parametrize("name", NAMES)
def test_fixture_conditions(name):
    """cond(G) <= 1e4, the smallest Cholesky pivot at least 1e3 x the engine's refusal threshold, and no minimum of a plain sweep decided by less than
    init_temporal_cases.MARGIN of the row's range"""
    c = sic.make(name)
    ref = sic.reference(name)
    for idx, res in ref["per_patch"].items():
        G = res["G"]
        cond = np.linalg.cond(G)
        piv = sio.cholesky_pivots(G)
        thr = sio.refusal_threshold(G)
        assert piv.size == G.shape[0] and cond <= 1e4 and piv.min() >= 1e3 * thr, (name, idx, cond, piv.min(), thr)
        pp = sio.ito.block_pixels(c.patch_pos[idx], c.d1)
        A = c.A.toarray().astype(np.float64)[pp][:, ref["ind"][idx]]
        margins, C12 = sio.sweep_min_margins(res["Ysig"], A, res["C0"], 12)
        assert np.array_equal(C12, res["C"]) and np.array_equal(C12, res["C_raw"])      # (ten sweeps and two more are twelve: the margins are those of the oracle's own run)
        assert margins.min() >= itc.MARGIN, (name, idx, margins.min())
