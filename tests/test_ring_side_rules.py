"""cnmf_e_amd/csrc/kept_results.hpp, option ring_side -- which residual requests may take the W*A tables a ring fit built on the side stream behind its solve
(ring_side_applies), without a GPU.  tests/ring_side_driver.cpp is built with the host compiler under the address and undefined-behaviour sanitizers and run as a
child process on a case file, the way tests/test_kept_results.py runs its driver; every combination is compared with a statement of the rule written here from
include/cnmfe.h (option ring_side) and DESIGN.md section 3, "Ring by-products beside the spatial update"."""
import itertools
import os
import shutil
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
B = (0, 1)


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("c++")
    if cxx is None:
        pytest.skip("no host C++ compiler")
    exe = str(tmp_path_factory.mktemp("ring_side") / "ring_side_driver")
    out = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-Wall", "-Wextra", "-Werror",
                          os.path.join(HERE, "ring_side_driver.cpp"), "-o", exe], capture_output=True, text=True)
    assert out.returncode == 0, out.stderr[-3000:]

    def run(command, cases):
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


def test_which_residual_requests_take_the_tables_built_behind_the_solve(driver):
    # ring_side, one lane, patches, the patch's W is final behind the solve's event, the request has footprints, a foreign buffer, tables only, Ysig wanted, recorded
    cases = list(itertools.product((0, 1, 2, 3), B, (1, 2), B, B, B, B, B, B))
    got = driver("ringside", cases)
    for (mode, one_lane, npatches, marked, has_ac, foreign, tables, want_out, recorded), (g,) in zip(cases, got):
        # "1 overlapped, 2 the join directly behind the scope, 0 off"; inert with lanes, with several patches, without the mark of a ring fit (the outlier
        # branch, bg_ssub's fits, anything that changed W since), for the low-resolution requests of bg_ssub and for every request that is not just recorded
        want = int(mode in (1, 2) and one_lane and npatches == 1 and marked and has_ac and not foreign and not tables and not want_out and recorded)
        assert g == want, (mode, one_lane, npatches, marked, has_ac, foreign, tables, want_out, recorded)
    assert sum(g for (g,) in got) == 2
