"""compactSpatial and trimSpatial on the NumPy engine double (the hostops path): against the oracle's circular_constraints per column and against the explicit-shift
restatement of trimSpatial in tests/image_ops_oracle.py, on the fixtures of tests/image_ops_cases.py."""
import os
import sys

import numpy as np
import pytest
import scipy.sparse as sp

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import cnmfe_oracle as orc
import image_ops_cases as ic
import image_ops_oracle as io
from cnmf_e_amd import hostops


def _sources(name, T=8, min_pixel=5):
    from fake_engine import FakeEngine
    from cnmf_e_amd.sources2d import PatchedVideo, Sources2D, Options
    c = ic.case(name)
    d1, d2, A = c["d1"], c["d2"], c["A"].copy()
    K = A.shape[1]
    video = PatchedVideo(d1, d2, T, [d1, d2], 3, FakeEngine())
    rng = np.random.default_rng(1)
    s = Sources2D(video, Options(ring_radius=3, min_pixel=min_pixel), A, rng.uniform(0, 1, (K, T)).astype(np.float32), np.ones(d1 * d2, np.float32))
    return s, c


@pytest.mark.parametrize("name", ic.NAMES)
def test_compact_spatial_equals_the_oracle(name):
    s, c = _sources(name)
    d1, d2 = c["d1"], c["d2"]
    A0 = c["A"].toarray().astype(np.float64)
    s.compactSpatial()
    got = s.A.toarray()
    for k in range(A0.shape[1]):
        ref = orc.circular_constraints(A0[:, k].reshape(d1, d2, order="F")).reshape(-1, order="F")
        assert np.array_equal(got[:, k], ref), (name, k)
    assert s.A.has_sorted_indices and not np.any(s.A.data == 0)


@pytest.mark.parametrize("name", ic.NAMES)
@pytest.mark.parametrize("thr,sz", [(0.01, 5), (0.2, 3), (0.01, 1)])
def test_trim_spatial_equals_the_explicit_restatement(name, thr, sz):
    s, c = _sources(name)
    ref, small_ref = io.trim_spatial(c["A"].toarray(), c["d1"], c["d2"], thr, sz, 5)
    small = s.trimSpatial(thr, sz)
    assert small.dtype == bool and np.array_equal(small, small_ref), name
    assert np.array_equal(s.A.toarray(), ref), name
    assert s.A.shape[1] == c["A"].shape[1]                               # (nothing is deleted)


def test_trim_spatial_branches_are_the_ones_the_fixture_names():
    """'opening': column 0 loses nothing (the opening removed everything), column 1 loses its raw maximum, column 2 keeps the brighter component only"""
    c = ic.case("opening")
    A0 = c["A"].toarray()
    got, small = hostops.trim_spatial(c["A"], c["d1"], c["d2"], 0.01, 5, 5)
    got = got.toarray()
    assert np.array_equal(got[:, 0], A0[:, 0])
    assert got[np.argmax(A0[:, 1]), 1] == 0 and np.count_nonzero(got[:, 1]) == 49
    assert np.count_nonzero(got[:, 2]) == 49 and got[:, 2].max() == 3.0
    assert not small.any()
    assert hostops.trim_spatial(c["A"], c["d1"], c["d2"], 0.01, 5, 50)[1].tolist() == [True, True, True]


def test_diagonal_lobes_differ_by_more_than_one_percent():
    for e1, e2 in ic.diagonal_lobe_energies():
        assert abs(e1 - e2) > 0.01 * max(e1, e2)


@pytest.mark.parametrize("sz", [0, 2, 4, 10, 11])
def test_even_or_out_of_range_sz_raises(sz):
    s, c = _sources("blobs")
    A = s.A
    with pytest.raises(ValueError):
        s.trimSpatial(0.01, sz)
    assert s.A is A
    with pytest.raises(ValueError):
        hostops.trim_spatial(c["A"], c["d1"], c["d2"], 0.01, sz, 5)


@pytest.mark.parametrize("call", ["compactSpatial", "trimSpatial"])
def test_only_A_is_replaced(call):
    s, c = _sources("blobs")
    s.A_prev = s.A.copy(); s.C_prev = np.asarray(s.C).copy()
    before = {k: v for k, v in vars(s).items() if k != "A"}
    A_old = s.A
    s._ind_future = (A_old, None)                                        # a mask prefetched for the old A ...
    before["_ind_future"] = s._ind_future
    getattr(s, call)()
    assert s.A is not A_old and (s.A != A_old).nnz > 0
    assert s._ind_future[0] is not s.A                                   # ... is not one _search_location_csc would take for the new A
    after = {k: v for k, v in vars(s).items() if k != "A"}
    assert before.keys() == after.keys()
    for k in before:
        assert before[k] is after[k], k
    assert np.array_equal(A_old.toarray(), c["A"].toarray())             # (the old matrix was not written to)


def test_device_flag_defaults_on_and_the_double_keeps_the_host_path():
    s, _ = _sources("blobs")
    assert s.image_ops_on_device is True and not s._image_ops_device(s.A)
    from cnmf_e_amd.engine import Engine
    assert Engine.supports_image_ops is True and Engine.IMAGE_OPS_MAX_BOX == ic.MAX_BOX
