"""The packed ring solve with the footprint corrections of all-zero factor blocks skipped (rsp_rank2, ring_solve_packed.hpp) against the weights of the
build that applied every correction to every tile: a skipped term is fma(x, +-0, t) = t for finite x, so the comparison is BITWISE.

* tests/golden/ring_solve_sparse_parent.npz holds, for the four fits of tests/solve_sparse_cases.py at ring radii 2, 5, 8 and 15 (1, 3, 4 and 6 blocks of 16
  ring pixels), the kept pixel rows of W as the parent commit computed them (scripts/make_solve_sparse_golden.py, run on the MI355X with that commit's
  library; never written by a later build);
* the CPU test restates the ring order in NumPy and shows that among the kept rows every way of skipping occurs: a neuron under the centre only, a footprint in
  one block, in some blocks, in all of them, more neurons than one staging round holds around one pixel, a ring cut by the border of the field of view -- so the
  fixture cannot pass by never skipping;
* the count each fit reports (pmax, fit_ring_model.m:60) equals max_i #{W(i, :) > 0} of the weights it started from: after a fit that solved every pixel, after
  a fit that left pixels inactive, and after ring_set_values."""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(ROOT, "oracle"))

import solve_sparse_cases as sc

GOLDEN = os.path.join(HERE, "golden", "ring_solve_sparse_parent.npz")


@pytest.fixture()
def eng():
    from cnmf_e_amd.engine import Engine
    e = Engine(0)
    yield e
    for k, v in (("solve_staged", 1), ("solve_inv", 0)):
        e.set_option(k, v)
    e.close()


@pytest.fixture(scope="module")
def golden():
    with np.load(GOLDEN) as z:
        return {k: z[k] for k in z.files}


@pytest.fixture(scope="module")
def inputs():
    return {r: sc.make_inputs(r) for r in sc.RADII}


def test_ring_order_is_the_oracles():
    import cnmfe_oracle as orc
    for r in sc.RADII:
        dr, dc = sc.ring_offsets(r)
        rs, cs = orc.get_nhood(r, None)
        assert np.array_equal(dr, rs) and np.array_equal(dc, cs)
    assert [(sc.ring_offsets(r)[0].size + 15) // 16 for r in sc.RADII] == [1, 3, 4, 6]


@pytest.mark.parametrize("r", sc.RADII)
def test_every_skip_class_occurs_among_the_kept_rows(r):
    rows = sc.sample_rows(r)
    small, wide = sc.census(r, sc.footprints(r, False), rows), sc.census(r, sc.footprints(r, True), rows)
    nt = small["nt"]
    print("radius %d, %d blocks, %d rows: small %s wide %s" % (r, nt, rows.size, small, wide))
    for cen in (small, wide):
        assert cen["centre_only"] > 0                        # mask 0: only the g update and nothing of rsp_rank2
        assert cen["one_block"] > 0
        assert cen["crowded"] > 0                            # a second staging round
    assert wide["all_blocks"] > 0                            # nothing skipped
    assert wide["border_live"] > 0 and (r == 2 or small["border_live"] > 0)
    if nt > 1:
        assert small["some_blocks"] > 0 and wide["some_blocks"] > 0
        assert small["all_blocks"] == 0                      # (without the wide footprint no neuron is spared the skipping)
        assert small["terms_kept"] < small["terms"] // 2
    assert sc.inactive_pixels(r, sc.footprints(r, False)) > 0 and sc.inactive_pixels(r, sc.footprints(r, True)) == 0


@pytest.mark.gpu
@pytest.mark.parametrize("staged", [1, 0])
@pytest.mark.parametrize("r", sc.RADII)
def test_sparse_corrections_are_bit_identical_to_the_parent(eng, inputs, golden, r, staged):
    from cnmf_e_amd.sources2d import PatchedVideo
    Y, fits = inputs[r]
    rows = sc.sample_rows(r)
    assert np.array_equal(golden["r%d_rows" % r], rows)
    eng.set_option("solve_staged", staged); eng.set_option("solve_inv", 0)
    video = PatchedVideo(sc.D1, sc.D2, sc.T, [sc.D1, sc.D2], r, eng)
    video.upload_from_full(Y)
    res = sc.run_fits(eng, r, fits)
    d = sc.D1 * sc.D2
    for k, (W, info, before) in enumerate(res):
        assert info["first_run"] == (k == 0) and np.all(np.isfinite(W.data))
        if before is not None:
            assert info["pmax"] == before, (r, k, info["pmax"], before)
        got, ref = sc.sampled_bits(W, rows), golden["r%d_fit%d" % (r, k)]
        assert got.shape == ref.shape
        diff = np.abs(got.view(np.float32).astype(np.float64) - ref.view(np.float32).astype(np.float64)).max() / float(golden["r%d_fit%d_maxabs" % (r, k)])
        print("radius %d fit %d staged %d: max |W - W_parent| / max |W_parent| = %.3g, active %d of %d" % (r, k, staged, diff, info["n_active"], d))
        assert np.array_equal(got, ref), (r, k, diff)
    assert res[0][1]["n_active"] == d and res[1][1]["n_active"] == d
    assert 0 < res[2][1]["n_active"] < d and 0 < res[3][1]["n_active"] < d          # (pixels without a footprint on their ring keep their weights -- and their count)
