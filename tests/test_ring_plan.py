"""cnmf_e_amd/csrc/ring_plan.hpp -- the pure host part of the ring fit's set-up (pair list, need masks, work and tile lists, footprint block lists, staged-window
metadata) -- without a GPU: tests/ring_plan_driver.cpp is built with the host compiler under the address and undefined-behaviour sanitizers, run as a child
process on a case file, and every table it prints is compared with its DEFINITION written out in NumPy (not a transcription of the C++ loops)."""
import os
import shutil
import subprocess

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
WIN_NLB, NWIN_MAX = 64, 32768


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("c++")
    if cxx is None:
        pytest.skip("no host C++ compiler")
    exe = str(tmp_path_factory.mktemp("ring_plan") / "ring_plan_driver")
    out = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-Wall", "-Wextra", "-Werror",
                          os.path.join(HERE, "ring_plan_driver.cpp"), "-o", exe], capture_output=True, text=True)
    assert out.returncode == 0, out.stderr[-3000:]

    def run(*commands):
        """one case file of commands (each a list of ints behind its name) -> per command a dict name -> int array"""
        case = exe + ".case"
        with open(case, "w") as fh:
            for c in commands:
                fh.write(" ".join(str(x) for x in c) + "\n")
        r = subprocess.run([exe, case], capture_output=True, text=True)
        assert r.returncode == 0, (r.returncode, r.stderr[-3000:])
        res, cur = [], {}
        for line in r.stdout.splitlines():
            name, *vals = line.split()
            if name == "end":
                res.append(cur); cur = {}
            else:
                cur[name] = np.array(vals, dtype=np.int64)
        assert len(res) == len(commands)
        return res
    return run


def ring(r):
    """offsets of the pixels with r <= distance < r + 1"""
    g = np.arange(-r - 1, r + 2)
    dc, dr = np.meshgrid(g, g, indexing="ij")
    dist = np.hypot(dr, dc)
    m = (dist >= r) & (dist < r + 1)
    return dr[m], dc[m]


def displacements(maxd):
    """the canonical block displacements (dR, dC) -- dC > 0, or dC = 0 and dR >= 0, both within maxd -- in the order of their index: by dC, then dR"""
    return [(dR, dC) for dC in range(maxd + 1) for dR in range(-maxd, maxd + 1) if dC > 0 or dR >= 0]


# (region rows, columns, patch row / column offset, patch rows, columns, ring radius, expected maxd)
GEOMS = {"a": (40, 36, 0, 0, 40, 36, 5, 1), "b": (47, 52, 15, 0, 32, 36, 15, 2), "c": (75, 66, 0, 0, 75, 66, 18, 3)}


@pytest.mark.parametrize("case", sorted(GEOMS))
def test_pair_need_work_and_tile_tables(driver, case):
    nr_b, nc_b, roff, coff, nr, nc, radius, maxd = GEOMS[case]
    dr, dc = ring(radius)
    p = dr.size
    if case == "c":
        assert (p + 15) // 16 == 8                               # (8 register tiles of ring neighbours)
    out = driver(["pairs", nr_b, nc_b, roff, coff, nr, nc, p, *dr, *dc])[0]
    R = int(max(np.abs(dr).max(), np.abs(dc).max()))
    disp = displacements(maxd)
    nrel = len(disp)
    assert list(out["reach"]) == [R, maxd, nrel, (2 * R) // 16 + 2, -(-R // 16), 1]
    nbr, nbc = -(-nr_b // 16), -(-nc_b // 16)
    # touched: the blocks that hold a pixel of the patch rectangle grown by the reach, clipped to the region
    ti = set(np.arange(max(0, roff - R), min(nr_b - 1, roff + nr - 1 + R) + 1) // 16)
    tj = set(np.arange(max(0, coff - R), min(nc_b - 1, coff + nc - 1 + R) + 1) // 16)
    want = {}
    for j in tj:
        for i in ti:
            for rel, (dR, dC) in enumerate(disp):
                if i + dR in ti and j + dC in tj:
                    want[(j * nbr + i, (j + dC) * nbr + i + dR)] = rel
    pairs = out["pairs"].reshape(-1, 4)
    assert {(a, b): rel for a, b, rel, _ in pairs.tolist()} == want and len(pairs) == len(want) and not pairs[:, 3].any()
    assert out["count"][0] == len(pairs)                         # (what bg_reserve sizes its tables by)
    pair_of = np.full(nbr * nbc * nrel, -1)
    pair_of[pairs[:, 0] * nrel + pairs[:, 2]] = np.arange(len(pairs))
    assert np.array_equal(out["pair_of"], pair_of)
    # needmask: bit (rel, pi, pj) iff a pixel of 4 x 4 sub-tile pi of a block and a pixel of sub-tile pj of the block `rel` away differ by an element of D
    O = set(zip(dr.tolist(), dc.tolist()))
    D = {(a - c, b - d) for a, b in O for c, d in O} | O | {(-a, -b) for a, b in O}
    M = 63 + 2 * R                                               # (two pixels of blocks <= 3 apart differ by at most 63)
    Dm = np.zeros((2 * M + 1, 2 * M + 1), bool)
    for a, b in D:
        Dm[a + M, b + M] = True
    four = np.arange(4)
    need = np.zeros((nrel, 16, 16), bool)
    for rel, (dR, dC) in enumerate(disp):
        for pi in range(16):
            ri, ci = (pi & 3) * 4 + four, (pi >> 2) * 4 + four
            for pj in range(16):
                rj, cj = (pj & 3) * 4 + 16 * dR + four, (pj >> 2) * 4 + 16 * dC + four
                rd, cd = np.subtract.outer(rj, ri).ravel(), np.subtract.outer(cj, ci).ravel()
                need[rel, pi, pj] = Dm[rd[:, None] + M, cd[None, :] + M].any() and not (rel == 0 and pi > pj)
    got = (out["needmask"].reshape(nrel, 16)[:, :, None] >> np.arange(16)) & 1
    assert np.array_equal(got.astype(bool), need)
    # work: the non-empty quadrants (pi half | pj half << 1) of every pair's mask, pair-major; tile lists: their sub-tiles as i | j << 4 in quadrant coordinates
    quad = lambda rel, q: need[rel, (q & 1) * 8:(q & 1) * 8 + 8, (q >> 1) * 8:(q >> 1) * 8 + 8]
    assert list(out["work"]) == [pp * 4 + q for pp, (_, _, rel, _) in enumerate(pairs.tolist()) for q in range(4) if quad(rel, q).any()]
    tl = out["tlist"].reshape(nrel, 4, 64)
    for rel in range(nrel):
        for q in range(4):
            i, j = np.nonzero(quad(rel, q))
            assert out["tcnt"][rel * 4 + q] == i.size
            assert list(tl[rel, q, :i.size]) == list(i | (j << 4)) and not tl[rel, q, i.size:].any()


def footprints(nr_b, nc_b, seed):
    """nine 7 x 7 blobs, one empty column, one footprint of two pixels in opposite corners: CSC over the region's pixels (column-major), as pixel lists too"""
    rng = np.random.default_rng(seed)
    pix = []
    for _ in range(9):
        r0, c0 = int(rng.integers(0, nr_b - 6)), int(rng.integers(0, nc_b - 6))
        pix.append([(r0 + a, c0 + b) for b in range(7) for a in range(7)])
    pix.insert(4, [])
    pix.append([(0, 0), (nr_b - 1, nc_b - 1)])
    return pix


def csc_args(pix, nr_b):
    colptr = np.cumsum([0] + [len(f) for f in pix])
    rowidx = [c * nr_b + r for f in pix for r, c in sorted(f, key=lambda rc: (rc[1], rc[0]))]
    return [len(pix), *colptr, *rowidx]


@pytest.mark.parametrize("case", sorted(GEOMS))
def test_block_lists_and_staged_windows(driver, case):
    nr_b, nc_b, _, _, _, _, radius, maxd = GEOMS[case]
    pix = footprints(nr_b, nc_b, 7 + ord(case))
    K = len(pix)
    out = driver(["lists", nr_b, nc_b, radius, *csc_args(pix, nr_b)])[0]
    assert out["maxd"][0] == maxd and out["ok"][0] == 1
    nbr, nbc = -(-nr_b // 16), -(-nc_b // 16)
    nblk = nbr * nbc
    # block b lists neuron k iff a footprint pixel of k lies in a block within Chebyshev distance maxd of b
    lists = [[] for _ in range(nblk)]
    for b in range(nblk):
        bi, bj = b % nbr, b // nbr
        for k, f in enumerate(pix):
            if any(max(abs(r // 16 - bi), abs(c // 16 - bj)) <= maxd for r, c in f):
                lists[b].append(k)                               # (ascending in k)
    lp = out["lst_ptr"]
    assert lp[0] == 0 and list(np.diff(lp)) == [len(l) for l in lists]
    assert list(out["lst_k"]) == [k for l in lists for k in l]
    slot = np.full((nblk, K), -1)
    for b, l in enumerate(lists):
        slot[b, l] = np.arange(len(l))
    assert np.array_equal(out["slot_of"].reshape(nblk, K), slot)
    # length classes (n - 1) >> 4 with ascending block inside; blall: a permutation of the non-empty blocks, longest class first
    classes = [[b for b in range(nblk) if lists[b] and (len(lists[b]) - 1) >> 4 == t] for t in range(4)]
    assert [list(out["nt%d" % t]) for t in range(4)] == classes
    assert list(out["blall"]) == classes[3] + classes[2] + classes[1] + classes[0]
    assert sorted(out["blall"]) == [b for b in range(nblk) if lists[b]]
    # the int8 window kernel's items: per block of blall one per PAIR of 16-trace groups of its list
    assert list(out["items"]) == [b | (g << 24) for b in out["blall"] for g in range((-(-len(lists[b]) // 16) + 1) // 2)]
    # staged windows: the bounding box grown by two reaches and clipped, the candidate box by one, offsets a running sum
    nbox, nmeta, tot = out["nbox"].reshape(K, 4), out["nmeta"].reshape(K, 8), 0
    for k, f in enumerate(pix):
        if not f:
            assert nbox[k, 1] < 0 and not nmeta[k].any()
            continue
        rr, cc = np.array(f).T
        box = [rr.min(), rr.max(), cc.min(), cc.max()]
        assert list(nbox[k]) == box
        grow = lambda m: (max(0, box[0] - m), min(nr_b - 1, box[1] + m), max(0, box[2] - m), min(nc_b - 1, box[3] + m))
        r0, r1, c0, c1 = grow(2 * radius)
        a0, a1, b0, b1 = grow(radius)
        assert list(nmeta[k]) == [r0, c0, r1 - r0 + 1, c1 - c0 + 1, tot, a0 | (a1 << 16), b0 | (b1 << 16), 0]
        tot += (r1 - r0 + 1) * (c1 - c0 + 1)
    assert out["stage"][0] == tot
    lmeta = out["lmeta"].reshape(-1, 8)
    assert np.array_equal(lmeta[:, 0], out["lst_k"]) and np.array_equal(lmeta[:, 1:], nmeta[out["lst_k"], :7])


def test_overflow_and_window_too_large(driver):
    """more than WIN_NLB neurons on one block's list: the overflow verdict and nothing else; a window above NWIN_MAX entries: the staged path declines"""
    rng = np.random.default_rng(3)
    q = rng.choice(256, 70, replace=False)
    pix = [[(16 + int(x) % 16, 16 + int(x) // 16)] for x in q]    # 70 one-pixel footprints inside block (1, 1) of a 40 x 36 region
    corners = [[(0, 0), (199, 179)]]
    over, large = driver(["lists", 40, 36, 5, *csc_args(pix, 40)], ["lists", 200, 180, 5, *csc_args(corners, 200)])
    assert 70 > WIN_NLB and over["ok"][0] == 0 and set(over) == {"maxd", "ok", "nbox"}
    assert 200 * 180 > NWIN_MAX and large["ok"][0] == 1 and large["stage"][0] == -1


def test_win_segments(driver):
    nbs = [1, 7, 255, 256, 511, 512, 4096]
    want = [max(1, min(8, (2048 + nb - 1) // nb)) if nb >= 512 else max(1, min(16, (4096 + nb - 1) // max(1, nb))) for nb in nbs]
    assert list(driver(["segments", len(nbs), *nbs])[0]["nsg"]) == want
