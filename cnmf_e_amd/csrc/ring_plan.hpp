// The host part of the ring fit's set-up (bg.hip) and of the spatial update's table (vproj.hip): pure integer table building, no HIP, no engine types -- plain
// ints and vectors in and out, so that tests/ring_plan_driver.cpp exercises it under the sanitizers without a GPU.  Every rule has ONE copy here; bg_reserve
// sizes its buffers from the same functions the fit runs.  Output orders are part of the contract (the kernels and the bit-for-bit tests rely on them): lists
// ascend in k, length classes run longest first with ascending block inside a class, work is pair-major.
#pragma once
#include <algorithm>
#include <cstdint>
#include <cstdlib>
#include <vector>
#ifdef __HIPCC__
#define RP_HD __host__ __device__ __forceinline__
#else
#define RP_HD inline
#endif

namespace cnmfe {
constexpr int WIN_NLB = 64;                           // list entries of one block the window kernels are built for
constexpr int NWIN_MAX = 32768;                       // entries of one neuron's window; a larger footprint sends the fit to k_ring_solve6
// canonical displacement index: dC in 0..maxd; dC == 0 -> dR in 0..maxd (0..maxd); dC >= 1 -> dR in -maxd..maxd.  maxd = 2: 13 classes (0..2, 3..7, 8..12)
RP_HD int rel_index(int dR, int dC, int maxd) { return dC == 0 ? dR : (maxd + 1) + (dC - 1) * (2 * maxd + 1) + dR + maxd; }
RP_HD int nrel_of(int maxd) { return (maxd + 1) + maxd * (2 * maxd + 1); }

namespace plan {
constexpr int B = 16;                                 // pixels per side of a block

// ---- ring reach: two ring pixels of one centre are up to 2*p_radius apart along an axis, their 16x16 blocks up to maxd apart (2 for radius <= 16, 3 up to 24) ----
// p_radius: largest |offset|; maxd: largest block displacement, nrel classes; nbw: blocks per side of the (2*radius+1)-pixel window; window origins reach -woff blocks;
// ok: the block-pair table covers it (offsets <= 24 pixels)
struct Reach { int p_radius, maxd, nrel, nbw, woff; bool ok; };
inline Reach ring_reach(const int *dr, const int *dc, int p) {
    Reach r{};
    for (int i = 0; i < p; ++i) r.p_radius = std::max(r.p_radius, std::max(std::abs(dr[i]), std::abs(dc[i])));
    r.maxd = (2 * r.p_radius + 15) >> 4; r.nrel = nrel_of(r.maxd); r.nbw = ((2 * r.p_radius) >> 4) + 2; r.woff = (r.p_radius + 15) >> 4;
    r.ok = r.maxd <= 3 && r.nbw <= 4;
    return r;
}
// frame segments per block of a window projection over nb blocks: enough workgroups to fill the chip; small patches (few blocks) get more, shorter segments
inline int win_segments(int nb) { return nb >= 512 ? std::max(1, std::min(8, (2048 + nb - 1) / nb)) : std::max(1, std::min(16, (4096 + nb - 1) / std::max(1, nb))); }

// ---- pair list: blocks that hold ring pixels of some patch pixel (or patch pixels), canonical displacement within +-maxd.  The patch is the nr x nc rectangle at
// (roff, coff) of the nr_b x nc_b block region.  Returns the count; pairs / pair_of (inverse index [block * nrel + rel], -1) are filled when given ----
struct Pair { int a, b, rel, pad; };                  // (the device reads them as int4)
inline int ring_pairs(int nr_b, int nc_b, int roff, int coff, int nr, int nc, int p_radius, int maxd, std::vector<Pair> *pairs, std::vector<int> *pair_of) {
    const int nbr = (nr_b + B - 1) / B, nbc = (nc_b + B - 1) / B, nrel = nrel_of(maxd);
    const int pi0 = std::max(0, roff - p_radius) / B, pi1 = std::min(nr_b - 1, roff + nr - 1 + p_radius) / B;      // the touched blocks: a rectangle
    const int pj0 = std::max(0, coff - p_radius) / B, pj1 = std::min(nc_b - 1, coff + nc - 1 + p_radius) / B;
    if (pairs) pairs->clear();
    if (pair_of) pair_of->assign((size_t)nbr * nbc * nrel, -1);
    int n = 0;
    for (int j = pj0; j <= pj1; ++j)
        for (int i = pi0; i <= pi1; ++i)
            for (int dC = 0; dC <= maxd; ++dC)
                for (int dR = (dC == 0 ? 0 : -maxd); dR <= maxd; ++dR) {
                    const int i2 = i + dR, j2 = j + dC;
                    if (i2 < pi0 || i2 > pi1 || j2 > pj1) continue;
                    const int rel = rel_index(dR, dC, maxd);
                    if (pair_of) (*pair_of)[(size_t)(j * nbr + i) * nrel + rel] = n;
                    if (pairs) pairs->push_back(Pair{j * nbr + i, j2 * nbr + i2, rel, 0});
                    ++n;
                }
    return n;
}

// ---- needed 16x16 sub-tiles per displacement class (displacement set D = (O - O) u O u -O of the ring offsets O), the work list and the tile lists ----
// needmask[rel * 16 + pi] bit pj: 4x4-pixel sub-tile pi of a block meets sub-tile pj of the block `rel` away; work: pair * 4 + quadrant, the non-empty ones;
// tcnt / tlist per (rel, quadrant): the needed sub-tiles as i | j << 4 (quadrant coordinates), 64 slots each
struct Tables { std::vector<unsigned short> needmask; std::vector<int> work, tcnt, tlist; };
inline void ring_tables(const std::vector<Pair> &pairs, int maxd, int p_radius, const int *dr, const int *dc, int p, Tables &t) {
    const int nrel = nrel_of(maxd), DB = 2 * p_radius, DM = 2 * DB + 1;
    std::vector<char> Dm((size_t)DM * DM, 0);
    auto dset = [&](int r, int c) { if (r >= -DB && r <= DB && c >= -DB && c <= DB) Dm[(size_t)(r + DB) * DM + c + DB] = 1; };
    for (int a = 0; a < p; ++a) {
        dset(dr[a], dc[a]); dset(-dr[a], -dc[a]);
        for (int b = 0; b < p; ++b) dset(dr[b] - dr[a], dc[b] - dc[a]);
    }
    t.needmask.assign((size_t)nrel * 16, 0);
    for (int dC = 0; dC <= maxd; ++dC)
        for (int dR = (dC == 0 ? 0 : -maxd); dR <= maxd; ++dR) {
            const int rel = rel_index(dR, dC, maxd);
            for (int pi = 0; pi < 16; ++pi)
                for (int pj = 0; pj < 16; ++pj) {
                    if (rel == 0 && pi > pj) continue;       // self pair: upper patch triangle (cov_lookup swaps)
                    const int ri = (pi & 3) * 4, ci = (pi >> 2) * 4, rj = (pj & 3) * 4 + dR * 16, cj = (pj >> 2) * 4 + dC * 16;
                    bool nd = false;
                    for (int x = -3; x <= 3 && !nd; ++x)
                        for (int y = -3; y <= 3; ++y) {
                            const int ddr = rj - ri + x, ddc = cj - ci + y;
                            if (ddr >= -DB && ddr <= DB && ddc >= -DB && ddc <= DB && Dm[(size_t)(ddr + DB) * DM + ddc + DB]) { nd = true; break; }
                        }
                    if (nd) t.needmask[rel * 16 + pi] |= (unsigned short)(1u << pj);
                }
        }
    // work order: pair-major (the displacement classes of one I block are consecutive), so heavy and light quadrants are mixed in time.  (Measured: class-major
    // order, which makes concurrent workgroups equal-cost, was slower -- 150 vs 131 ms at 512x512x10000 -- and did not raise the L2 hit rate.)
    t.tcnt.assign((size_t)nrel * 4, 0); t.tlist.assign((size_t)nrel * 4 * 64, 0);
    for (int rel = 0; rel < nrel; ++rel)
        for (int q = 0; q < 4; ++q) {
            const int ih = q & 1, jh = q >> 1;
            int n = 0;
            for (int i = 0; i < 8; ++i) for (int j = 0; j < 8; ++j)
                if ((t.needmask[rel * 16 + ih * 8 + i] >> (jh * 8 + j)) & 1) t.tlist[(size_t)(rel * 4 + q) * 64 + n++] = i | (j << 4);
            t.tcnt[rel * 4 + q] = n;
        }
    t.work.clear();
    for (size_t pp = 0; pp < pairs.size(); ++pp)
        for (int q = 0; q < 4; ++q) if (t.tcnt[pairs[pp].rel * 4 + q]) t.work.push_back((int)pp * 4 + q);
}

// ---- the blocks near each footprint: per column k of a CSC matrix over the nr_b-row block region, the blocks within maxd of a block that holds one of its entries
// (pair_blk[k_ptr[k] .. k_ptr[k + 1])), and its bounding box nbox[4 k ..]: first / last row, first / last column.  Flat arrays, two passes, reused scratch: a vector
// of vectors cost 0.4 ms of allocator churn per fit at the headline size, in front of the window projection ----
inline void footprint_blocks(int K, const int64_t *colptr, const int32_t *rowidx, int nr_b, int nbr, int nbc, int maxd, std::vector<int> &pair_blk, std::vector<int> &k_ptr,
                             std::vector<int> &nbox) {
    static thread_local std::vector<int> own, seen, mark;
    own.assign((size_t)nbr * nbc, -1); seen.assign((size_t)nbr * nbc, -1);
    pair_blk.clear(); k_ptr.assign((size_t)K + 1, 0); nbox.assign((size_t)4 * std::max(1, K), 0);
    for (int k = 0; k < K; ++k) {
        mark.clear();
        int bx[4] = {1 << 30, -1, 1 << 30, -1};
        // (the entries of a column ascend with the pixel index: one step per run of an image column of the block region, not per entry)
        for (int64_t e = colptr[k]; e < colptr[k + 1];) {
            const int q0 = rowidx[e], cb = q0 / nr_b, col_end = (cb + 1) * nr_b;
            int qlast = q0;
            ++e;
            while (e < colptr[k + 1] && rowidx[e] < col_end && rowidx[e] >= qlast) { qlast = rowidx[e]; ++e; }
            bx[0] = std::min(bx[0], q0 - cb * nr_b); bx[1] = std::max(bx[1], qlast - cb * nr_b); bx[2] = std::min(bx[2], cb); bx[3] = std::max(bx[3], cb);
            for (int bi = (q0 - cb * nr_b) >> 4; bi <= (qlast - cb * nr_b) >> 4; ++bi) {
                const int b_ = (cb >> 4) * nbr + bi;
                if (own[b_] != k) { own[b_] = k; mark.push_back(b_); }
            }
        }
        for (int i = 0; i < 4; ++i) nbox[(size_t)4 * k + i] = bx[i];
        for (int b_ : mark)
            for (int dj = -maxd; dj <= maxd; ++dj)
                for (int di = -maxd; di <= maxd; ++di) {
                    const int i2 = b_ % nbr + di, j2 = b_ / nbr + dj;
                    if (i2 < 0 || i2 >= nbr || j2 < 0 || j2 >= nbc) continue;
                    if (seen[j2 * nbr + i2] != k) { seen[j2 * nbr + i2] = k; pair_blk.push_back(j2 * nbr + i2); }
                }
        k_ptr[k + 1] = (int)pair_blk.size();
    }
}

// ---- from k-major (block, neuron) pairs to the lists the window kernels read: lst_k[lst_ptr[b] ..) ascending in k, slot_of[b * K + k] = position or -1, the
// non-empty blocks by length class (n - 1) >> 4 and all of them longest class first.  false: some block lists more than WIN_NLB neurons (nothing else is valid) ----
struct BlockLists { std::vector<int> lst_ptr, lst_k, blk_nt[4], blall; std::vector<short> slot_of; };
inline bool block_lists(int nblk, int K, const int *pair_blk, const int *k_ptr, BlockLists &L) {
    static thread_local std::vector<int> fill;
    fill.assign(nblk, 0);
    for (int i = 0; i < k_ptr[K]; ++i) ++fill[pair_blk[i]];
    L.lst_ptr.assign((size_t)nblk + 1, 0);
    for (int b = 0; b < nblk; ++b) {
        if (fill[b] > WIN_NLB) return false;
        L.lst_ptr[b + 1] = L.lst_ptr[b] + fill[b];
        fill[b] = 0;                                       // (from here: next free slot)
    }
    L.lst_k.resize(k_ptr[K]);
    L.slot_of.assign((size_t)nblk * std::max(1, K), (short)-1);
    for (int k = 0; k < K; ++k)
        for (int i = k_ptr[k]; i < k_ptr[k + 1]; ++i) {
            const int b = pair_blk[i], s_ = fill[b]++;
            L.lst_k[L.lst_ptr[b] + s_] = k; L.slot_of[(size_t)b * K + k] = (short)s_;
        }
    for (auto &v : L.blk_nt) v.clear();
    for (int b = 0; b < nblk; ++b) if (fill[b]) L.blk_nt[(fill[b] - 1) >> 4].push_back(b);
    L.blall.clear();
    for (int t = 3; t >= 0; --t) L.blall.insert(L.blall.end(), L.blk_nt[t].begin(), L.blk_nt[t].end());
    return true;
}
// the work items of the int8 window kernel: (block | group << 24), one per pair of 16-trace groups of a block's list, blocks in blall's order
inline void win_i8_items(const std::vector<int> &blall, const std::vector<int> &lst_ptr, std::vector<int> &items) {
    items.clear();
    for (int b : blall) {
        const int ntl = (lst_ptr[b + 1] - lst_ptr[b] + 15) >> 4;
        for (int gq = 0; gq < (ntl + 1) / 2; ++gq) items.push_back(b | (gq << 24));
    }
}

// ---- staged windows (ring_solve_staged.hpp): per neuron 8 ints -- origin row, column, rows, columns, offset of its dense window, then the candidate box as
// lo | hi << 16 for rows and for columns -- and per list position the neuron and its seven.  A centre whose ring reaches the footprint lies within one radius of its
// bounding box (the candidate test), and that ring's pixels within two: U~ = Yc Cc' - ... is non-zero wherever the video is, and the correction pairs it with A on
// ANOTHER ring pixel.  Returns the windows' total entries, or -1: a window above NWIN_MAX (or 2^30 entries in all) ----
inline int64_t stage_windows(int K, const std::vector<int> &nbox, const std::vector<int> &lst_k, int nr_b, int nc_b, int p_radius, std::vector<int> &nmeta, std::vector<int> &lmeta) {
    nmeta.assign((size_t)8 * K, 0); lmeta.assign((size_t)8 * std::max<size_t>(1, lst_k.size()), 0);
    int64_t tot = 0;
    for (int k = 0; k < K; ++k) {
        const int *bx = &nbox[(size_t)4 * k];
        int *mk = &nmeta[(size_t)8 * k];
        if (bx[1] < 0) continue;                           // (an empty footprint: on no list)
        const int R2 = 2 * p_radius;
        const int r0 = std::max(0, bx[0] - R2), r1 = std::min(nr_b - 1, bx[1] + R2), c0 = std::max(0, bx[2] - R2), c1 = std::min(nc_b - 1, bx[3] + R2);
        mk[5] = std::max(0, bx[0] - p_radius) | (std::min(nr_b - 1, bx[1] + p_radius) << 16);
        mk[6] = std::max(0, bx[2] - p_radius) | (std::min(nc_b - 1, bx[3] + p_radius) << 16);
        const int64_t n = (int64_t)(r1 - r0 + 1) * (c1 - c0 + 1);
        if (n > NWIN_MAX || tot + n > ((int64_t)1 << 30)) return -1;
        mk[0] = r0; mk[1] = c0; mk[2] = r1 - r0 + 1; mk[3] = c1 - c0 + 1; mk[4] = (int)tot;
        tot += n;
    }
    for (size_t i = 0; i < lst_k.size(); ++i) {
        lmeta[8 * i] = lst_k[i];
        for (int j = 0; j < 7; ++j) lmeta[8 * i + 1 + j] = nmeta[(size_t)8 * lst_k[i] + j];
    }
    return tot;
}
}  // namespace plan
}  // namespace cnmfe
