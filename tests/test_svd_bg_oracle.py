"""The float64 oracle of background_model = 'svd' (tests/svd_bg_oracle.py) against numpy.linalg.svd, and the well-posedness of the test cases."""
import numpy as np
import pytest
import scipy.sparse as sp

import cnmfe_oracle as orc
import svd_bg_cases as sc
import svd_bg_oracle as so


def _blocks(case):
    pp, bp = orc.distribute_geometry(case["d1"], case["d2"], case["patch"], case["halo"])
    d1 = case["d1"]
    for idx in np.ndindex(pp.shape):
        p, b = [int(x) for x in pp[idx]], [int(x) for x in bp[idx]]
        rows = np.arange(b[0] - 1, b[1]); cols = np.arange(b[2] - 1, b[3])
        pix = (cols[None, :] * d1 + rows[:, None]).reshape(-1, order="F")
        yield idx, pix, orc.ind_patch_mask(pp[idx], bp[idx]).reshape(-1)


@pytest.mark.parametrize("shape", [(30, 70), (70, 30)])          # both branches of svdsecon: X X' (m <= n) and X' X
@pytest.mark.parametrize("nb", [1, 3])
def test_svdsecon_equals_numpy_svd(shape, nb):
    rng = np.random.default_rng(5)
    X = rng.normal(size=shape) + 5 * np.outer(rng.normal(size=shape[0]), rng.normal(size=shape[1]))
    U, s, V = so.svdsecon(X, nb)
    Un, sn, Vtn = np.linalg.svd(X, full_matrices=False)
    assert np.allclose(s, sn[:nb], rtol=1e-10)
    assert np.allclose((U * s) @ V.T, (Un[:, :nb] * sn[:nb]) @ Vtn[:nb], atol=1e-9 * sn[0])
    assert np.allclose(U.T @ U, np.eye(nb), atol=1e-9) and np.allclose(V.T @ V, np.eye(nb), atol=1e-9)


@pytest.mark.parametrize("name,neurons", sc.CASES)
@pytest.mark.parametrize("nb", [1, 2, 3])
def test_cases_are_well_posed_and_fit_equals_svd(name, neurons, nb):
    case = sc.make_case(name, nb, neurons)
    seen_empty = False
    for idx, pix, ip in _blocks(case):
        Yb, ind, A_b, C_b = sc.block_inputs(case, pix)
        seen_empty |= ind.size == 0
        for with_a in [bool(ind.size)]:                                         # K = 0: the A = ones, C = zeros branch
            A_use, C_use = (A_b, C_b) if with_a else (None, None)
            sv = so.singular_values(Yb, A_use, C_use)
            gap, tail = sc.well_posed(sv, nb)
            print(name, neurons, nb, idx, "sigma_nb/sigma_nb+1 = %.1f  sigma_17/sigma_nb = %.3g" % (gap, tail))
            assert gap >= 3 and tail <= 0.5, (name, nb, idx, gap, tail)
            b, f, b0 = so.fit_svd_model(Yb, nb, A_use, C_use, ind_patch=ip)
            assert b.shape == (int(ip.sum()), nb) and f.shape == (nb, case["T"]) and b0.shape == (int(ip.sum()),)
            # against numpy's SVD of the same matrix: the product b f, never the factors singly
            Ad = np.zeros((Yb.shape[0], 1)) if A_use is None else A_use.toarray().astype(np.float64)
            Cd = np.zeros((1, case["T"])) if C_use is None else C_use.astype(np.float64)
            Bf = (Yb - Yb.mean(axis=1, keepdims=True)) - Ad @ (Cd - Cd.mean(axis=1, keepdims=True))
            U, s, Vt = np.linalg.svd(Bf - Bf.mean(axis=1, keepdims=True), full_matrices=False)
            ref = (U[:, :nb] * s[:nb]) @ Vt[:nb]
            assert np.abs(b @ f - ref[ip]).max() <= 1e-9 * s[0], (name, nb, idx)
            assert np.allclose(f @ f.T, np.eye(nb), atol=1e-9)
            assert np.allclose(b0, Yb.mean(axis=1)[ip] - (Ad @ Cd.mean(axis=1))[ip] - b @ f.mean(axis=1), atol=1e-9)
            # the background it explains: the planted components dominate what is left
            resid = Yb[ip] - (b @ f + b0[:, None]) - (Ad @ Cd)[ip]
            assert resid.std() <= 3 * sc.NOISE, (name, nb, idx, resid.std())
    assert seen_empty == (not neurons or name == "quad")                        # quad: the two right-hand blocks hold no neuron


def test_nb_zero_branch():
    case = sc.make_case("one", 0)
    _, pix, ip = next(_blocks(case))
    Yb, ind, A_b, C_b = sc.block_inputs(case, pix)
    b, f, b0 = so.fit_svd_model(Yb, 0, A_b, C_b, ind_patch=ip)
    assert b.shape == (ip.sum(), 0) and f.shape == (0, case["T"])
    assert np.allclose(b0, Yb.mean(axis=1) - A_b.astype(np.float64) @ C_b.astype(np.float64).mean(axis=1))
    b, f, b0 = so.fit_svd_model(Yb, 0, None, None, ind_patch=ip)
    assert np.allclose(b0, Yb.mean(axis=1))


def test_outlier_arguments_are_dead():
    """fit_svd_model.m:29 tests a misspelt variable: thresh_outlier, sn, b_old and f_old never change the fit"""
    case = sc.make_case("small", 2)
    _, pix, ip = next(_blocks(case))
    Yb, ind, A_b, C_b = sc.block_inputs(case, pix)
    a = so.fit_svd_model(Yb, 2, A_b, C_b, ind_patch=ip)
    rng = np.random.default_rng(2)
    b = so.fit_svd_model(Yb, 2, A_b, C_b, b_old=rng.normal(size=a[0].shape), f_old=rng.normal(size=a[1].shape), thresh_outlier=0.1, sn=np.full(ip.sum(), 0.01), ind_patch=ip)
    for x, y in zip(a, b):
        assert np.array_equal(x, y)


def test_ind_patch_selects_the_interior_of_the_block():
    case = sc.make_case("quad", 1)
    for idx, pix, ip in _blocks(case):
        assert 0 < ip.sum() < ip.size                                   # a strict interior: the halo is fitted and dropped
        Yb, ind, A_b, C_b = sc.block_inputs(case, pix)
        full = so.fit_svd_model(Yb, 1, A_b if ind.size else None, C_b if ind.size else None)
        part = so.fit_svd_model(Yb, 1, A_b if ind.size else None, C_b if ind.size else None, ind_patch=ip)
        assert np.allclose(full[0][ip] @ full[1], part[0] @ part[1], atol=1e-9 * np.abs(full[0]).max()) and np.allclose(full[2][ip], part[2])
    assert sp.issparse(case["A"])
