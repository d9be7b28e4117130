"""The ring solve's diagonal step with the inverse half shared between the four DPP rows (cnmf_e_amd/csrc/ring_solve_core.hpp, rs_inv) against the weights
the replicated form computed: every element sees the same operations on the same values, so the comparison is BITWISE.

* golden fits: tests/golden/ring_solve_w_parent.npz holds, for the fits of tests/solve_valu_cases.py (48 x 48, T = 300, K = 8, a first-run fit and a fit with
  the true footprints, ring radii with 1 .. 6 tiles of 16 ring pixels), a seeded sample of 128 pixel rows of W as the parent commit computed them
  (scripts/make_solve_golden.py, run on the MI355X with that commit's library);
* crowded pixel: twelve footprints on one pixel's ring -- more than a staging round holds -- with solve_staged = 0 and 1: bitwise equal to each other, and within
  the 2e-6 of the parity tests of the float64 oracle;
* the count the next fit reports (pmax, fit_ring_model.m:60) equals max_i #{W(i, :) > 0} of the weights fetched before it, also when the fit left pixels inactive.
  The count is still k_ring_pmax's pass over W (api.hip): the solve kernels do not count in their epilogue, so these assertions pin the existing kernel.
The lane model of the new layout (scripts/ring_solve5_model.py) is checked on the CPU at the end of this file."""
import os
import sys

import numpy as np
import pytest
import scipy.sparse as sp

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(ROOT, "oracle"))
sys.path.insert(0, os.path.join(ROOT, "scripts"))

import solve_valu_cases as sc

GOLDEN = os.path.join(HERE, "golden", "ring_solve_w_parent.npz")


@pytest.fixture()
def eng():
    from cnmf_e_amd.engine import Engine
    e = Engine(0)
    yield e
    for k, v in (("solve_staged", 1), ("solve_inv", 0), ("solve_probe", 0)):
        e.set_option(k, v)
    e.close()


@pytest.fixture(scope="module")
def inputs():
    return sc.make_inputs()


@pytest.fixture(scope="module")
def golden():
    with np.load(GOLDEN) as z:
        return {k: z[k] for k in z.files}


def _video(eng, Y, r):
    from cnmf_e_amd.sources2d import PatchedVideo
    video = PatchedVideo(sc.D1, sc.D2, sc.T, [sc.D1, sc.D2], r, eng)
    video.upload_from_full(Y)
    return video


def _pmax(W):
    """max_i #{W(i, :) > 0} (fit_ring_model.m:60)"""
    Wc = W.tocsr()
    return int(np.asarray((Wc > 0).sum(axis=1)).max())


def test_the_radii_instantiate_every_tile_count():
    assert {sc.ring_tiles(r) for r in sc.RADII} == {1, 2, 3, 4, 5, 6}


@pytest.mark.gpu
@pytest.mark.parametrize("staged", [1, 0])
@pytest.mark.parametrize("r", sc.RADII)
def test_golden_fits_are_bit_identical_to_the_parent(eng, inputs, golden, r, staged):
    """k_ring_solve8 (staged = 1) and k_ring_solve6 (0) share the core: both must reproduce the parent's bits.  The third fit repeats the second's inputs on the
    weights the second left and checks the count it reports against them; at the small radii most pixels of that fit are inactive."""
    Y, fits = inputs
    assert np.array_equal(golden["rows"], sc.sample_rows())
    eng.set_option("solve_staged", staged); eng.set_option("solve_inv", 0)
    video = _video(eng, Y, r)
    res = sc.run_fits(eng, video, r, fits + [fits[1]])
    d = sc.D1 * sc.D2
    for k, (W, info) in enumerate(res):
        assert info["first_run"] == (k == 0) and np.all(np.isfinite(W.data))
        if k > 0:
            assert info["pmax"] == _pmax(res[k - 1][0]), (r, k, info["pmax"], _pmax(res[k - 1][0]))
        if k < 2:
            got, ref = sc.sampled_bits(W, golden["rows"]), golden["r%d_fit%d" % (r, k)]
            assert got.shape == ref.shape
            diff = np.abs(got.view(np.float32).astype(np.float64) - ref.view(np.float32).astype(np.float64)).max() / float(golden["r%d_fit%d_maxabs" % (r, k)])
            print("radius %d fit %d staged %d: max |W - W_parent| / max |W_parent| = %.3g, active %d of %d" % (r, k, staged, diff, info["n_active"], d))
            assert np.array_equal(got, ref), (r, k, diff)
    assert res[0][1]["n_active"] == d
    if r <= 3:
        assert 0 < res[1][1]["n_active"] < d and 0 < res[2][1]["n_active"] < d        # (pixels without a footprint on their ring keep their weights -- and their count)


@pytest.mark.gpu
def test_crowded_pixel_takes_a_second_staging_round(eng):
    import cnmfe_oracle as orc
    from parity_util import rel
    r = 15
    Y, A, C = sc.crowded_inputs()
    rs, cs = orc.get_nhood(r, None)
    D = A.toarray().reshape(sc.D1, sc.D2, -1, order="F")
    on_ring = set()
    for dr, dc in zip(rs, cs):
        on_ring |= set(np.nonzero(D[24 + int(dr), 24 + int(dc)])[0].tolist())
    assert len(on_ring) > 8                                                              # more than RSP_NS (ring_solve_packed.hpp)
    video = _video(eng, Y, r)
    W0 = orc.build_ring_W(video.patch_pos[(0, 0)], video.block_pos[(0, 0)], sc.D1, sc.D2, rs, cs).tocsr(); W0.sort_indices()
    out = {}
    for staged in (0, 1):
        eng.set_option("solve_staged", staged); eng.set_option("solve_inv", 0)
        Ws = []
        for W, info in sc.run_fits(eng, video, r, [(A, C), ((A * 0.8).tocsc().astype(np.float32), C)]):
            assert np.all(np.isfinite(W.data))
            if Ws:
                assert info["pmax"] == _pmax(Ws[-1])
            Ws.append(W)
        out[staged] = Ws
    for wa, wb in zip(out[0], out[1]):
        assert np.array_equal(wa.data.view(np.uint32), wb.data.view(np.uint32))
    W_old = W0
    for k, sca in enumerate((1.0, 0.8)):
        Ak = (A * sca).tocsc().astype(np.float32)
        Wr, _ = orc.fit_ring_model(Y.T.astype(np.float64), Ak.astype(np.float64), C, W_old, np.nan, None, np.ones(sc.D1 * sc.D2, bool), True)
        Wr = sp.csr_matrix(Wr); Wr.sort_indices()
        e = rel(out[1][k].data, Wr.data)
        print("crowded fit %d: rel err against the oracle %.3g" % (k, e))
        assert e <= 2e-6, (k, e)
        W_old = Wr


def test_lane_model_of_the_shared_inverse_half():
    """CPU: the 64-lane model of the diagonal step -- column cc of the inverse half in DPP row cc & 3, slot s in the register of a[s] -- against the one-row model
    (bitwise) and NumPy's Cholesky and inverse of random SPD 16 x 16 blocks"""
    import ring_solve5_model as m
    worst = m.check_diag_block_rows(np.random.default_rng(3), n=12)
    assert worst < 1e-10, worst
