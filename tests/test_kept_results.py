"""cnmf_e_amd/csrc/kept_results.hpp -- the host rules of the results that outlive a call: the record of a deferred spatial update (KeptSpatial) and the two
predicates of the hand-over between the spatial and the temporal update (early_takes, early_serves) -- without a GPU.  tests/kept_results_driver.cpp is built
with the host compiler under the address and undefined-behaviour sanitizers and run as a child process on a case file.  EVERY combination is enumerated and
compared with

* a statement of the rules written here from what include/cnmfe.h says (cnmfe_update_spatial and its fetch calls; option temporal_early,
  cnmfe_temporal_early_project, cnmfe_temporal_early_claim), and
* the boolean expressions of factor.hip as they stood before the rules moved (the driver's legacy_* commands), on the loose fields the context had then.

The driver's `lanestate` command moves a LaneState-shaped struct of stub buffers (a host stand-in with the move operations of DevBuf and PinArena): the source
is left empty, every allocation is released exactly once."""
import itertools
import os
import shutil
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
B = (0, 1)
OFF, DECLINED, YES = 0, 1, 2


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("c++")
    if cxx is None:
        pytest.skip("no host C++ compiler")
    exe = str(tmp_path_factory.mktemp("kept_results") / "kept_results_driver")
    out = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-Wall", "-Wextra", "-Werror",
                          os.path.join(HERE, "kept_results_driver.cpp"), "-o", exe], capture_output=True, text=True)
    assert out.returncode == 0, out.stderr[-3000:]

    def run(command, cases):
        """one line `command args...` per case -> one tuple of ints per case"""
        path = exe + ".case"
        with open(path, "w") as fh:
            for c in cases:
                fh.write(command + " " + " ".join(str(int(x)) for x in c) + "\n")
        r = subprocess.run([exe, path], capture_output=True, text=True)
        assert r.returncode == 0, (r.returncode, r.stderr[-3000:])
        rows = [tuple(int(x) for x in line.split()) for line in r.stdout.splitlines()]
        assert len(rows) == len(cases)
        return rows
    return run


# ---- early_takes ------------------------------------------------------------------------------------------------------------------------------------------------
# temporal_early, then per tag field 1 = equal to the update's own (claimed token, patch, K, row stride, T, spatial generation, request generation), nnz(A),
# the residual is a recorded request | of cnmfe_residual, one lane, the pending term has the update's stride, then the three projection options equal
TAKE_CASES = list(itertools.product((0, 1, 2, 3), B, B, B, B, B, B, B, (0, 5), B, B, B, B, B, B, B))


def takes_rule(mode, claimed, P, K, ldc, T, sgen, rgen, nnz, virt, full, one_lane, terms, i8, planes, tiled):
    # "temporal_early: 1 (default) both halves, 2 the projection only, 3 the levels only, 0 off" -- the projection is the half asked about
    if mode not in (1, 2):
        return 0
    # cnmfe_temporal_early_claim: "the A of the next cnmfe_hals_temporal IS the result the token was given for"; without the claim nothing is taken
    if not claimed:
        return 0
    # "taken only when every field of the tag still holds": same patch, K, T (and the row stride that follows from it), no spatial update and no residual request since
    if not (P and K and ldc and T and sgen and rgen):
        return 0
    # the projection was computed from the centred video under a recorded request of cnmfe_residual, on one lane, for a non-empty A whose pending term goes
    # through the projection (else the term is folded into Ysig and the request is no longer virtual)
    if not (nnz > 0 and virt and full and one_lane and terms):
        return 0
    # "... and by the kernel the options select now": proj_i8, proj_i8_planes, proj_tiled as they were when it was queued
    return int(i8 and planes and tiled)


def test_early_takes_over_the_full_product(driver):
    assert len(TAKE_CASES) == 4 * 2 ** 7 * 2 * 2 ** 4 * 2 ** 3
    got = driver("takes", TAKE_CASES)
    bad = [(c, g) for c, g in zip(TAKE_CASES, got) if g != (takes_rule(*c),)]
    assert not bad, (len(bad), bad[:5])
    assert sum(g[0] for g in got) == 2                                       # (temporal_early = 1 and 2 with everything equal: nothing else is taken)
    assert got == driver("legacy_takes", TAKE_CASES)


# ---- early_serves -----------------------------------------------------------------------------------------------------------------------------------------------
# temporal_early, one lane, the record names a patch, its K equals the request's, nnz of the request, the record's nnz equals it, the keep flags are in place,
# of the latest spatial result, the patch is the field of view, its residual is a recorded request | of cnmfe_residual
SERVE_CASES = list(itertools.product((0, 1, 2, 3), B, B, B, (0, 5), B, B, B, B, B, B))


def serves_rule(mode, one_lane, has_patch, K, nnz, nnz_eq, flags, gen_eq, fov, virt, full):
    # "*token = 0 when the request is declined"; with the option off or several lanes the call does nothing and counts nothing
    if mode not in (1, 2) or not one_lane:
        return OFF
    # the result of the last deferred spatial update must still lie on the device with its keep flags (the connected fetch ran, nothing took a slot since),
    # be non-empty, be the one the caller describes (K, nnz) and belong to a patch that still exists
    if not (has_patch and K and nnz > 0 and nnz_eq and flags and gen_eq):
        return DECLINED
    # "declined: a patch that is not the field of view, no virtual residual, bg_ssub > 1"
    if not (fov and virt and full):
        return DECLINED
    return YES


def test_early_serves_over_the_full_product(driver):
    assert len(SERVE_CASES) == 4 * 2 ** 3 * 2 * 2 ** 6
    got = driver("serves", SERVE_CASES)
    bad = [(c, g) for c, g in zip(SERVE_CASES, got) if g != (serves_rule(*c),)]
    assert not bad, (len(bad), bad[:5])
    assert {g[0] for g in got} == {OFF, DECLINED, YES} and sum(g[0] == YES for g in got) == 2
    assert got == driver("legacy_serves", SERVE_CASES)


# ---- KeptSpatial transitions ------------------------------------------------------------------------------------------------------------------------------------
SPATIAL5, SPATIAL0, CONNECTED, DROP, DROP_PATTERN, PATCH_GONE = 1, 2, 3, 4, 5, 6
KEPT_CASES = [c for n in range(0, 5) for c in itertools.product((SPATIAL5, SPATIAL0, CONNECTED, DROP, DROP_PATTERN, PATCH_GONE), repeat=n)]


def kept_rule(ops):
    """-> (fetch of 5 values serves, connected fetch of 5, fetch of 0 values, connected fetch of 0, a hand-over request finds the result), from include/cnmfe.h:
    the deferred result is valid until the next spatial, temporal, fast-temporal or post-processing call on the lane (DROP); the connected fetch also needs the
    mask's pattern, which cnmfe_deconv_temporal takes (DROP_PATTERN); the hand-over needs the keep flags of the latest result and its patch"""
    nnz, pattern, flags, patch = None, False, False, False
    for op in ops:
        if op in (SPATIAL5, SPATIAL0):
            nnz, pattern, flags, patch = (5 if op == SPATIAL5 else 0), op == SPATIAL5, False, True
        elif op == CONNECTED:
            flags = flags or (nnz == 5 and pattern)
        elif op == DROP:
            nnz, pattern, flags, patch = None, False, False, False
        elif op == DROP_PATTERN:
            pattern = flags = False
        elif op == PATCH_GONE:
            patch = False
    return int(nnz == 5), int(nnz == 5 and pattern), int(nnz == 0), int(nnz == 0), int(patch and flags)


def test_kept_spatial_transitions(driver):
    assert len(KEPT_CASES) == sum(6 ** n for n in range(5))
    cases = [c if c else (0,) for c in KEPT_CASES]                         # (0: no operation)
    got = driver("kept", cases)
    bad = [(c, g, kept_rule(c)) for c, g in zip(cases, got) if g != kept_rule(c)]
    assert not bad, (len(bad), bad[:5])
    assert {g for g in got} >= {(1, 1, 0, 0, 1), (1, 1, 0, 0, 0), (1, 0, 0, 0, 0), (0, 0, 1, 1, 0), (0, 0, 0, 0, 0)}
    # the fields the record replaced (spatial_nnz, spatial_patch, conn_gen == spatial_gen) went through the same states wherever no call took a slot: the two
    # deliberate differences are exactly DROP (the parent kept serving the fetch) and DROP_PATTERN (the parent kept serving the connected fetch)
    legacy = driver("legacy_kept", cases)
    for c, g, l in zip(cases, got, legacy):
        if DROP not in c and DROP_PATTERN not in c:
            assert g == l, (c, g, l)
        else:
            assert g[4] <= l[4] and all(a <= b for a, b in zip(g, l)), (c, g, l)   # (never served where the parent refused)
    assert any(g != l for g, l in zip(got, legacy))


# ---- a lane's state changes places as a whole -------------------------------------------------------------------------------------------------------------------
def test_lane_state_moves_leave_the_source_empty(driver):
    got = driver("lanestate", [(0,), (1,), (2,), (3,)])
    # (ok, allocations alive while the lanes exist, alive after they went): one lane's worth after a move, two after a swap, none at the end
    per_lane = 3 + 1 + 4 + 12 + 1 + 1                                      # arena + its two events, bf, vp[4], every second scr slot, tmp[1], dscr.pw
    assert got == [(1, per_lane, 0), (1, per_lane, 0), (1, 2 * per_lane, 0), (1, 2 * per_lane, 0)], got
