"""The fits of tests/test_gpu_solve_sparse.py and of scripts/make_solve_sparse_golden.py (which recorded tests/golden/ring_solve_sparse_parent.npz with them).

The packed ring solve skips the footprint corrections of a tile whose factor block of 16 ring pixels holds no footprint pixel (rsp_rank2, ring_solve_packed.hpp).
These footprints are laid out so that every way of skipping occurs among the pixel rows the fixture keeps, at every ring radius:
  * twelve small footprints centred on ring pixels of the middle pixel (24, 24): more neurons around that pixel than one staging round holds (RSP_NS = 8); for the
    pixels near them, footprints in one block, in a few blocks, and -- for the pixel under a footprint's middle -- in none (the ring passes the footprint by);
  * two lone footprints near two corners, so that rings cut by the border of the field of view carry corrections too;
  * in the second fit only, one footprint that covers the whole field of view: every block of every ring, nothing to skip, every pixel active.
Four fits per radius: the first run, the fit with the wide footprint, a fit that leaves pixels inactive, and a fit on weights set with ring_set_values."""
import numpy as np
import scipy.sparse as sp

D1, D2, T, SEED = 48, 48, 300, 23
MID = (24, 24)
RADII = (2, 5, 8, 15)                          # 16, 40, 56, 96 ring pixels -> NT = 1, 3, 4, 6 blocks of 16
HALF = {2: 0, 5: 1, 8: 1, 15: 2}               # half width of the small footprints: the ring of the pixel under a footprint's middle must pass it by
NSMALL = 12
LONE = ((5, 41), (42, 7))
RSP_NS = 8                                     # ring_solve_packed.hpp
NRAND, ROW_SEED = 96, 20261


def ring_offsets(R):
    """the ring of fit_ring_model in the kernels' order: R^2 <= dr^2 + dc^2 < (R + 1)^2, sorted by (dc, dr)"""
    v = np.arange(-R - 1, R + 2)
    dc, dr = [x.ravel() for x in np.meshgrid(v, v, indexing="ij")]
    d2 = dr * dr + dc * dc
    keep = (d2 >= R * R) & (d2 < (R + 1) * (R + 1))
    dr, dc = dr[keep], dc[keep]
    o = np.lexsort((dr, dc))
    return dr[o], dc[o]


def small_centres(R):
    dr, dc = ring_offsets(R)
    idx = np.round(np.linspace(0, dr.size, NSMALL, endpoint=False)).astype(int)
    return [(MID[0] + int(dr[i]), MID[1] + int(dc[i])) for i in idx] + list(LONE)


def footprints(R, wide):
    """d x K float32 CSC: the small footprints of radius R, then the wide one"""
    from cnmf_e_amd import synth
    cen = small_centres(R)
    h = HALF[R]
    amp = np.random.default_rng(SEED + R).uniform(0.5, 1.5, len(cen))
    A = synth._footprints(D1, D2, cen, amp, max(h, 1) * 0.75, 2 * h + 1)
    if wide:
        A = sp.hstack([A, synth._footprints(D1, D2, [(20.0, 27.0)], [0.7], 30.0, 2 * max(D1, D2) + 1)])
    return A.tocsc().astype(np.float32)


def make_inputs(R):
    """the video (T x d, float32) and the (A, C) of the fits"""
    from cnmf_e_amd import synth
    K = NSMALL + len(LONE)
    f = synth.make_factors(D1, D2, T, K + 1, SEED, gSig=1.5, gSiz=5, min_sep=3)
    f.A_true = footprints(R, True); f.A_init = f.A_true
    Y = synth.make_video(f, np.float32)
    C = np.ascontiguousarray(f.C_init, dtype=np.float32)
    A_small, A_wide = footprints(R, False), footprints(R, True)
    A_dim = (A_small * 0.8).tocsc().astype(np.float32)
    return Y, [(A_small, C[:K]), (A_wide, C), (A_dim, C[:K]), (A_dim, C[:K])]


def sample_rows(R):
    """pixel rows of W the fixture keeps: the middle pixel, the pixels under the small footprints' middles, the corners and border pixels beside the lone
    footprints, and a seeded sample of the rest"""
    forced = [MID, (0, 0), (D1 - 1, D2 - 1), (0, D2 - 1), (D1 - 1, 0)] + small_centres(R)
    for (r, c) in LONE:
        forced += [(min(max(r + a, 0), D1 - 1), min(max(c + b, 0), D2 - 1)) for a in (-R, 0, R) for b in (-R, 0, R)]
    rows = {c * D1 + r for (r, c) in forced}
    rows |= set(np.random.default_rng(ROW_SEED).choice(D1 * D2, size=NRAND, replace=False).tolist())
    return np.array(sorted(rows), dtype=np.int64)


def set_values(W):
    """what the last fit starts from: the weights of the fit before with every third sign flipped (ring_set_values)"""
    v = np.array(W.data, dtype=np.float32, copy=True)
    v[::3] = -np.abs(v[::3])
    return v


def pmax_of(W):
    """max_i #{W(i, :) > 0} (fit_ring_model.m:60)"""
    return int(np.asarray((W.tocsr() > 0).sum(axis=1)).max())


def run_fits(eng, R, fits, pid=0):
    """ring_init + the four fits; per fit (W as CSR, info of the fit, pmax of the weights the fit started from or None)"""
    eng.ring_init(pid, R)
    out = []
    for k, (A, C) in enumerate(fits):
        before = None
        if k == 3:
            v = set_values(out[-1][0])
            eng.ring_set_values(pid, v)
            Wb = out[-1][0].copy(); Wb.data = v
            before = pmax_of(Wb)
        elif k > 0:
            before = pmax_of(out[-1][0])
        _, info = eng.fit_ring_model(pid, A, C)
        out.append((eng.ring_csr(pid), info, before))
    return out


def sampled_bits(W, rows):
    return np.ascontiguousarray(W[rows].data, dtype=np.float32).view(np.uint32)


def census(R, A, rows):
    """NumPy model of what the kernels skip, over the pixel rows `rows`: per (pixel, neuron) with a footprint pixel on the ring or under the centre, the mask of
    the blocks of 16 ring pixels that hold one.  Returns a dict of counts per class."""
    dr, dc = ring_offsets(R)
    nt = (dr.size + 15) // 16
    D = np.asarray(A.toarray() != 0).reshape(D1, D2, -1, order="F")
    blk = np.arange(dr.size) // 16
    out = dict(nt=nt, centre_only=0, one_block=0, some_blocks=0, all_blocks=0, crowded=0, border_live=0, pairs=0, terms=0, terms_kept=0)
    for m in rows:
        r, c = int(m % D1), int(m // D1)
        rr, cc = r + dr, c + dc
        inside = (rr >= 0) & (rr < D1) & (cc >= 0) & (cc < D2)
        on = np.zeros((dr.size, D.shape[2]), bool)
        on[inside] = D[rr[inside], cc[inside]]
        live = 0
        for k in range(D.shape[2]):
            bits = np.unique(blk[on[:, k]])
            if bits.size == 0 and not D[r, c, k]:
                continue
            live += 1
            n = bits.size
            out["pairs"] += 1
            out["centre_only"] += n == 0
            out["one_block"] += n == 1
            out["some_blocks"] += 1 < n < nt
            out["all_blocks"] += n == nt
            # tile (I, J), I >= J: the term with alpha(J) and the term with alpha(I)
            out["terms"] += nt * (nt + 1)
            out["terms_kept"] += sum((J in bits) + (I in bits) for J in range(nt) for I in range(J, nt))
        out["crowded"] += live > RSP_NS
        out["border_live"] += (not inside.all()) and live > 0
    return out


def inactive_pixels(R, A):
    """pixels no footprint pixel of A lies on the ring of: a later fit leaves their weights alone (ind_active, fit_ring_model.m:28, for weights without zeros)"""
    dr, dc = ring_offsets(R)
    S = np.asarray(A.sum(axis=1)).ravel().reshape(D1, D2, order="F") != 0
    pad = np.zeros((D1 + 2 * (R + 1), D2 + 2 * (R + 1)), bool)
    pad[R + 1:R + 1 + D1, R + 1:R + 1 + D2] = S
    hit = np.zeros((D1, D2), bool)
    for a, b in zip(dr, dc):
        hit |= pad[R + 1 + a:R + 1 + a + D1, R + 1 + b:R + 1 + b + D2]
    return int((~hit).sum())
