"""The image operations on single footprints on the engine (csrc/footprint_ops.hpp) against cnmf_e_amd.hostops on the fixtures of tests/image_ops_cases.py.
Exact equality is the bound: every step of the three operations is a comparison, a selection or a correctly rounded fp64 operation in the host statement's order.
hostops itself is tied to the oracle by tests/test_hostops.py and tests/test_image_ops_host.py."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import scipy.sparse as sp

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, os.path.join(ROOT, "oracle"))
sys.path.insert(0, HERE)
pytestmark = pytest.mark.gpu

import image_ops_cases as ic
from cnmf_e_amd import hostops

ASYM = np.array([[1, 0, 0, 0, 0], [0, 1, 1, 0, 0], [0, 0, 1, 1, 1]], dtype=bool)        # an element that is neither symmetric nor square
ELEMENTS = {"disk1": hostops.strel_disk(1), "disk2": hostops.strel_disk(2), "disk4": hostops.strel_disk(4), "asym": ASYM}


@pytest.fixture(scope="module")
def eng():
    from cnmf_e_amd.engine import Engine
    e = Engine(0)
    yield e
    e.close()


@pytest.fixture(scope="module")
def host():
    """the hostops results, computed once per (operation, case, parameters)"""
    memo = {}

    def get(op, name, *par):
        key = (op, name) + tuple(p if not isinstance(p, np.ndarray) else p.tobytes() + bytes(p.shape) for p in par)
        if key not in memo:
            c = ic.case(name)
            A, d1, d2 = c["A"], c["d1"], c["d2"]
            if op == "circular":
                memo[key] = hostops.circular_constraints_columns(A, d1, d2)
            elif op == "dilate":
                memo[key] = hostops.search_location_dilate(A, d1, d2, par[0], c["nb"], par[1])
            else:
                memo[key] = hostops.trim_spatial(A, d1, d2, par[0], par[1], 5)
        return memo[key]
    return get


def same_matrix(got, ref):
    """values AND pattern"""
    got = sp.csc_matrix(got); ref = sp.csc_matrix(ref)
    got.sort_indices(); ref.sort_indices()
    return (got.shape == ref.shape and got.dtype == ref.dtype and np.array_equal(got.indptr, ref.indptr) and np.array_equal(got.indices, ref.indices)
            and np.array_equal(got.data, ref.data))


# ---- kernel parity -----------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ic.NAMES)
def test_circular_equals_hostops(eng, host, name):
    c = ic.case(name)
    got = eng.circular_constraints(c["A"], c["d1"], c["d2"])
    assert eng.counter("image_ops_host_columns") == c["host_columns"]
    assert same_matrix(got, host("circular", name)), name


@pytest.mark.parametrize("name", ic.NAMES)
def test_dilate_equals_hostops(eng, host, name):
    c = ic.case(name)
    se = hostops.strel_disk(4)
    got = eng.search_dilate(c["A"], c["d1"], c["d2"], se, c["nb"], 0.99)
    assert eng.counter("image_ops_host_columns") == c["host_columns"]
    assert same_matrix(got, host("dilate", name, se, 0.99)), name


@pytest.mark.parametrize("name", ic.NAMES)
def test_trim_equals_hostops(eng, host, name):
    c = ic.case(name)
    got, small = eng.trim_spatial(c["A"], c["d1"], c["d2"], 0.01, 5, 5)
    assert eng.counter("image_ops_host_columns") == c["host_columns"]
    ref, small_ref = host("trim", name, 0.01, 5)
    assert same_matrix(got, ref), name
    assert small.dtype == bool and np.array_equal(small, small_ref)


# ---- structural variants -----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["blobs", "borders", "diagonal", "nb2"])
@pytest.mark.parametrize("nrgthr", [0.99, 0.5])
@pytest.mark.parametrize("se", sorted(ELEMENTS))
def test_dilate_elements_and_thresholds(eng, host, name, nrgthr, se):
    c = ic.case(name)
    got = eng.search_dilate(c["A"], c["d1"], c["d2"], ELEMENTS[se], c["nb"], nrgthr)
    assert same_matrix(got, host("dilate", name, ELEMENTS[se], nrgthr)), (name, nrgthr, se)


def test_dilate_element_the_kernel_does_not_take_goes_to_the_host(eng, host):
    """an even side (and a side above the margin the box provides): every non-empty column is hostops', the result is the same"""
    c = ic.case("blobs")
    for se in (np.ones((2, 3), dtype=bool), hostops.strel_disk(8)):
        got = eng.search_dilate(c["A"], c["d1"], c["d2"], se, 1, 0.99)
        assert eng.counter("image_ops_host_columns") == c["A"].shape[1]
        assert same_matrix(got, hostops.search_location_dilate(c["A"], c["d1"], c["d2"], se, 1, 0.99))


@pytest.mark.parametrize("name", ["blobs", "borders", "opening", "diagonal"])
@pytest.mark.parametrize("thr,sz", [(0.01, 5), (0.2, 3), (0.01, 1)])
def test_trim_variants(eng, host, name, thr, sz):
    c = ic.case(name)
    got, small = eng.trim_spatial(c["A"], c["d1"], c["d2"], thr, sz, 5)
    ref, small_ref = host("trim", name, thr, sz)
    assert same_matrix(got, ref) and np.array_equal(small, small_ref), (name, thr, sz)


# ---- determinism -------------------------------------------------------------------------------------------------------------------------------------------
def _all_three(e, name):
    c = ic.case(name)
    a = e.circular_constraints(c["A"], c["d1"], c["d2"])
    b = e.search_dilate(c["A"], c["d1"], c["d2"], hostops.strel_disk(4), c["nb"], 0.99)
    t, small = e.trim_spatial(c["A"], c["d1"], c["d2"], 0.01, 5, 5)
    return a, b, t, small


def test_two_calls_and_two_lanes_are_bit_identical(eng):
    from cnmf_e_amd.engine import Engine
    e2 = Engine(0)
    try:
        e2.set_option("lanes", 2)
        for name in ("blobs", "borders"):
            first, again, lanes2 = _all_three(eng, name), _all_three(eng, name), _all_three(e2, name)
            for x, y, z in zip(first[:3], again[:3], lanes2[:3]):
                assert same_matrix(x, y) and same_matrix(x, z)
                assert x.data.tobytes() == y.data.tobytes() == z.data.tobytes()
            assert np.array_equal(first[3], again[3]) and np.array_equal(first[3], lanes2[3])
    finally:
        e2.close()


# ---- end to end --------------------------------------------------------------------------------------------------------------------------------------------
def _iterate(on_device):
    from cnmf_e_amd import synth
    from cnmf_e_amd.engine import Engine
    from cnmf_e_amd.sources2d import PatchedVideo, Sources2D, Options
    d1, d2, T, K, r = 40, 36, 128, 5, 3
    f = synth.make_factors(d1, d2, T, K, 23, gSig=2.0, gSiz=9, min_sep=6)
    Y = synth.make_video(f, np.float32)
    e = Engine(0)
    try:
        video = PatchedVideo(d1, d2, T, [d1, d2], r, e)
        video.upload_from_full(Y)
        s = Sources2D(video, Options(ring_radius=r, spatial_algorithm="hals", maxIter=3, search_method="dilate", bSiz=2,
                                     spatial_constraints={"circular": True, "connected": True}), f.A_init, f.C_init, f.sn)
        s.image_ops_on_device = on_device
        used = [s._image_ops_device(s.A)]
        for _ in range(2):
            s.update_background_parallel(); s.update_spatial_parallel(); s.update_temporal_parallel()
        used.append(s._image_ops_device(s.A))
        W = s.get_W(video.owned[0])
        out = dict(A=s.A.copy(), C=np.asarray(s.C, dtype=np.float32).copy(), W=(W.indptr.copy(), W.indices.copy(), W.data.copy()),
                   b0=np.array(s.b0_new, dtype=np.float64), used=used)
        A2 = s.A.copy()
        s.compactSpatial()
        out["compact"] = (s.A.copy(), hostops.circular_constraints_columns(A2, d1, d2))
        A3 = s.A.copy()
        small = s.trimSpatial()
        out["trim"] = (s.A.copy(), small, hostops.trim_spatial(A3, d1, d2, 0.01, 5, int(np.ceil(s.options.min_pixel))))
        s.update_background_parallel()                                   # the next fit runs on the replaced A
        e.synchronize()
        out["b0_next"] = np.array(s.b0_new, dtype=np.float64)
        return out
    finally:
        e.close()


def test_iterations_are_bit_identical_with_and_without_the_device_path():
    dev, hst = _iterate(True), _iterate(False)
    assert dev["used"] == [True, True] and hst["used"] == [False, False]      # (the first run did take the kernels: A is fp32 from the start)
    assert dev["A"].nnz > 0 and same_matrix(dev["A"], hst["A"])
    assert dev["C"].tobytes() == hst["C"].tobytes()
    for x, y in zip(dev["W"], hst["W"]):
        assert x.tobytes() == y.tobytes()
    assert dev["b0"].tobytes() == hst["b0"].tobytes()
    for run in (dev, hst):
        assert same_matrix(*run["compact"])
        A_t, small, (ref, small_ref) = run["trim"]
        assert same_matrix(A_t, ref) and np.array_equal(small, small_ref)
        assert np.all(np.isfinite(run["b0_next"]))
    assert dev["b0_next"].tobytes() == hst["b0_next"].tobytes()


# ---- the existing entry point ------------------------------------------------------------------------------------------------------------------------------
def test_post_process_spatial_is_what_it_was(eng):
    """cnmfe_post_process_spatial on case 1 against the oracle's connectivity_constraint, as tests/test_gpu_parity.py::test_post_process_spatial_parity does"""
    import cnmfe_oracle as orc
    c = ic.case("blobs")
    d1, d2, A = c["d1"], c["d2"], c["A"]
    got = eng.post_process_spatial(A, d1, d2).toarray()
    ref = orc.post_process_spatial(A.toarray().astype(np.float64).reshape(d1, d2, A.shape[1], order="F"))
    assert np.array_equal(got != 0, ref != 0)
    assert np.array_equal(got.astype(np.float64), ref)


# ---- refusals ----------------------------------------------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_context_usable(eng, host):
    from cnmf_e_amd import _lib as L
    from cnmf_e_amd.engine import _p
    c = ic.case("blobs")
    d1, d2 = c["d1"], c["d2"]
    d, K = d1 * d2, 2
    cp = np.array([0, 2, 3], dtype=np.int64); va = np.ones(3, dtype=np.float32)
    box = np.zeros((K, 4), dtype=np.int32); off = np.zeros(K + 1, dtype=np.int64); hc = np.zeros(K, dtype=np.uint8)
    keep = np.zeros(3, dtype=np.uint8); small = np.zeros(K, dtype=np.uint8); se = np.ones((3, 3), dtype=np.uint8)
    good = np.array([1, 5, 7], dtype=np.int32)

    def circ(ri):
        return L.lib.cnmfe_circular_constraints(eng._ctx, d1, d2, K, _p(cp, L.i64p), _p(ri, L.i32p), _p(va, L.f32p), _p(box, L.i32p), _p(off, L.i64p),
                                                C.cast(None, L.f32p), 0, _p(hc, L.u8p), L.HOST)

    def dil(ri, nrgthr):
        return L.lib.cnmfe_search_dilate(eng._ctx, d1, d2, K, _p(cp, L.i64p), _p(ri, L.i32p), _p(va, L.f32p), _p(se, L.u8p), 3, 3, 1, nrgthr, _p(box, L.i32p),
                                         _p(off, L.i64p), C.cast(None, L.u8p), 0, _p(hc, L.u8p), L.HOST)

    def trim(ri, sz):
        return L.lib.cnmfe_trim_spatial(eng._ctx, d1, d2, K, _p(cp, L.i64p), _p(ri, L.i32p), _p(va, L.f32p), 0.01, sz, 5, _p(keep, L.u8p), _p(small, L.u8p),
                                        _p(hc, L.u8p), L.HOST)
    EINVAL = -1                                                          # CNMFE_EINVAL (include/cnmfe.h)
    for bad in (np.array([1, d, 7], dtype=np.int32), np.array([-1, 5, 7], dtype=np.int32), np.array([5, 1, 7], dtype=np.int32), np.array([5, 5, 7], dtype=np.int32)):
        assert circ(bad) == EINVAL and dil(bad, 0.99) == EINVAL and trim(bad, 5) == EINVAL
    for sz in (0, 2, 4, 10, 11):
        assert trim(good, sz) == EINVAL
    for nrgthr in (0.0, -0.5, 1.5, float("nan")):
        assert dil(good, nrgthr) == EINVAL
    assert circ(good) == 0 and dil(good, 1.0) == 0 and trim(good, 5) == 0
    with pytest.raises(ValueError):
        eng.trim_spatial(c["A"], d1, d2, 0.01, 4, 5)
    assert same_matrix(eng.circular_constraints(c["A"], d1, d2), host("circular", "blobs"))
