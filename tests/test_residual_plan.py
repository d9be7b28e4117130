"""cnmf_e_amd/csrc/residual_plan.hpp -- the host rules of the residual: what a request does to the state beside Ysig, which kernel the sweep takes, whether a
footprint term can go through a projection -- without a GPU.  tests/residual_plan_driver.cpp is built with the host compiler under the address and
undefined-behaviour sanitizers and run as a child process on a case file.  EVERY combination is enumerated (the unreachable ones too: a residual of the other
kind in the patch, a RESIDENT form without a buffer, terms set beside a state without a pending term) and compared with

* a statement of the rules written here from what include/cnmfe.h says each option does (cnmfe_residual, cnmfe_residual_ssub, cnmfe_set_option), and
* the boolean expressions of resid.hip, ssub.hip and factor.hip as they stood before the rules moved (the driver's legacy_* commands)."""
import itertools
import os
import shutil
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
NONE, VIRTUAL, RESIDENT = 0, 1, 2
FULL, SSUB = 1, 2
PEND_ONLY, PEND_AND_FOLD, RECORD, SWEEP = 0, 1, 2, 3
B = (0, 1)


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("c++")
    if cxx is None:
        pytest.skip("no host C++ compiler")
    exe = str(tmp_path_factory.mktemp("residual_plan") / "residual_plan_driver")
    out = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-Wall", "-Wextra", "-Werror",
                          os.path.join(HERE, "residual_plan_driver.cpp"), "-o", exe], capture_output=True, text=True)
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


# ---- residual_plan ------------------------------------------------------------------------------------------------------------------------------------------
PLAN_CASES = list(itertools.product((NONE, VIRTUAL, RESIDENT), (0, FULL, SSUB), B,        # the state: form, who wrote it, Ysig buffer allocated
                                    (FULL, SSUB), B, B, B, B,                             # the request: cnmfe_residual | _ssub, has_ac, output wanted, outbuf, tables_only
                                    B, B, B, (0, 1, 2), (5 * 10**8 - 1, 5 * 10**8)))     # r1_delta, r1_lazy, r1_virtual, ssub_virtual, samples d_b T


def plan_rule(form, source, buffer, qsource, has_ac, want, outbuf, tables_only, delta, lazy, virt, sv, samples):
    """-> (action, reuse, virt_new, tables), from include/cnmfe.h"""
    ssub = qsource == SSUB
    # tables: the low-resolution patch builds W A and the centred traces only -- for cnmfe_residual that is the caller's word (tables_only, whatever the state),
    # cnmfe_residual_ssub asks it of its low-resolution patch exactly when no sweep is due
    tables = lambda no_sweep: no_sweep if ssub else tables_only
    if not ssub and outbuf:
        # the low-resolution patch of a cnmfe_residual_ssub: it sweeps into the caller's buffer or only builds its tables; its own residual plays no part
        return SWEEP, 0, 0, tables_only
    # "While the video, W and b0 of the patch are unchanged, a further call only changes the footprint term": a residual of the same call is kept -- as Ysig in
    # the patch's buffer or as a recorded request -- and option r1_delta is on
    if delta and form != NONE and source == qsource and (form == VIRTUAL or buffer):
        # "... folded into the resident Ysig in one streaming pass (r1_delta), or merely recorded (r1_lazy)"; an output buffer reads Ysig, so the term is folded
        return (PEND_ONLY if lazy and not want else PEND_AND_FOLD), 1, 0, tables(1)
    # r1_virtual / ssub_virtual: a request WITHOUT an output buffer is recorded; its term pends beside it, so r1_lazy and r1_delta must be on as well;
    # ssub_virtual: "2 always, 1 (default) on patches of at least 5e8 samples, 0: the low-resolution sweep + upsample"
    record = not want and virt and lazy and delta
    if ssub:
        record = record and (sv == 2 or (sv == 1 and samples >= 5e8))
    if record:
        return RECORD, 0, 1, tables(1)
    return SWEEP, 0, 0, tables(0)


def test_residual_plan_over_the_full_product(driver):
    assert len(PLAN_CASES) == 3 * 3 * 2 * 2 * 2 ** 4 * 2 ** 3 * 3 * 2
    got = driver("plan", PLAN_CASES)
    bad = [(c, g, plan_rule(*c)) for c, g in zip(PLAN_CASES, got) if g != tuple(int(x) for x in plan_rule(*c))]
    assert not bad, (len(bad), bad[:5])
    # every action occurs, for both requests
    for q in (FULL, SSUB):
        assert {g[0] for c, g in zip(PLAN_CASES, got) if c[3] == q} == {PEND_ONLY, PEND_AND_FOLD, RECORD, SWEEP}
    # a request of cnmfe_residual_ssub does not look at outbuf / tables_only, and has_ac never changes a plan
    by = {c: g for c, g in zip(PLAN_CASES, got)}
    for c, g in by.items():
        assert by[c[:4] + (1 - c[4],) + c[5:]] == g
        if c[3] == SSUB:
            assert by[c[:6] + (0, 0) + c[8:]] == g


def test_residual_plan_equals_the_expressions_it_replaced(driver):
    assert driver("plan", PLAN_CASES) == driver("legacy_plan", PLAN_CASES)


# ---- r1_kernel_plan -----------------------------------------------------------------------------------------------------------------------------------------
KERNEL_CASES = list(itertools.product((5, 6, 7, 8, 9, 15, 18), B, B, B, (-1, 3, 10, 11, 14), B, B))   # radius, full_ring, has_ac, can_defer, r1_variant, r1_lazy, r1_defer
GENERIC, DMA, ARC, DUO = -1, 10, 11, 14
TILE = {DMA: (32, 16), ARC: (16, 32), DUO: (32, 32)}


def kernel_rule(radius, full_ring, has_ac, can_defer, variant, lazy, defer):
    """-> (kernel or None, special, small_special, TR, TC, defer_term, sweep_ac, duo_segments)"""
    asked = variant if variant in (GENERIC, DMA, ARC, DUO) else DUO          # (r1_variant: 14 the default where it applies, -1 the generic kernel; unknown -> default)
    # r1_defer: "ring radius 15, no Ysig_out: the first residual after a fit also runs its sweep without the footprint term and leaves the term pending" -- so that the
    # duo-role kernel (which takes no term) serves; the term pends, so r1_lazy must be on
    defer_term = bool(has_ac and can_defer and lazy and defer and asked == DUO and radius == 15 and full_ring)
    sweep_ac = bool(has_ac and not defer_term)
    small = bool(full_ring and radius in (5, 6, 8, 9) and asked != GENERIC)  # the low-resolution rings of bg_ssub = 2, 3: LDS-DMA kernel only
    special = small or bool(full_ring and radius in (15, 18) and asked != GENERIC)
    kernel = None
    if small or (special and radius == 18):
        kernel = DMA                                                         # (the arc and duo kernels are built for radius 15)
    elif special:
        kernel = ARC if asked == DUO and sweep_ac else asked                 # (the duo kernel takes no footprint term inside the sweep)
    tr, tc = TILE[kernel] if special else (16, 16)
    duo_segments = asked == DUO and radius == 15 and not sweep_ac            # (the segmenting of 1024-pixel tiles goes with the request, whichever kernel runs)
    return kernel, special, small, tr, tc, defer_term, sweep_ac, duo_segments


def test_r1_kernel_plan(driver):
    got = driver("kernel", KERNEL_CASES)
    for c, g in zip(KERNEL_CASES, got):
        kernel, *rest, duo_segments = kernel_rule(*c)
        assert g[1:] == tuple(int(x) for x in rest), (c, g, rest)
        assert (g[0] == DUO) == duo_segments, (c, g)
        if rest[0]:
            assert g[0] == kernel, (c, g, kernel)
        elif c[4] == GENERIC:
            assert g[0] < 0, (c, g)
    assert {g[0] for g in got if g[1]} == {DMA, ARC, DUO} and any(g[5] for g in got)
    assert got == driver("legacy_kernel", KERNEL_CASES)


# ---- the predicates over the two terms ----------------------------------------------------------------------------------------------------------------------
KS = (512, 513, 8192, 8193, 65536, 65537)
TERM_CASES = list(itertools.product(B, B, (64, 68), KS, B, (64, 68), KS, (64,), (1, 8)))   # has_pending | pending: ac, ldc, K | applied: ac, ldc, K | ldc, K of the projection


def terms_rule(has_pending, pend_ac, pend_ldc, pend_K, res_ac, res_ldc, res_K, ldc, K):
    if not has_pending:
        return 1, 1, 1, 0                                                    # nothing differs from Ysig: every projection serves, nothing can overflow
    part = [(k, l) for ac, k, l in ((pend_ac, pend_K, pend_ldc), (res_ac, res_K, res_ldc)) if ac]      # the terms whose buffers are read
    match = pend_ldc == ldc and all(l == ldc for _, l in part)               # (the pending term's stride is the request's own: it counts with or without footprints)
    projectable = all(k <= 8192 and l == ldc for k, l in part)               # trace ids within the bitmap of k_term_project
    foldable = all(l == ldc and k * K <= 65536 for k, l in part)             # K_term x K inner products
    overflow = any(k > 512 for k, _ in part)                                 # more traces than the list of k_term_project holds
    return int(match), int(projectable), int(foldable), int(overflow)


def test_term_predicates_at_their_boundaries(driver):
    got = driver("terms", TERM_CASES)
    bad = [(c, g, terms_rule(*c)) for c, g in zip(TERM_CASES, got) if g != terms_rule(*c)]
    assert not bad, (len(bad), bad[:5])
    assert 8192 * 8 == 65536 * 1 == 65536 < 65537 * 1 < 8193 * 8                           # (both sides of FOLD_MAX_PAIRS are in the product)
    assert got == driver("legacy_terms", TERM_CASES)
