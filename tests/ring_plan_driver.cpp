// Stand-alone driver of cnmf_e_amd/csrc/ring_plan.hpp for tests/test_ring_plan.py: reads commands from a case file, prints every table as integers.
// Built with the host compiler and the address / undefined-behaviour sanitizers; no GPU, no HIP.
//   segments n nb...                                                     -> nsg
//   pairs nr_b nc_b roff coff nr nc p dr[p] dc[p]                        -> reach count pairs pair_of needmask work tcnt tlist
//   lists nr_b nc_b p_radius K colptr[K + 1] rowidx[nnz]                 -> maxd ok lst_ptr lst_k slot_of nt0..nt3 blall items nbox stage nmeta lmeta
#include "../cnmf_e_amd/csrc/ring_plan.hpp"
#include <cstdio>
#include <fstream>
#include <iostream>
#include <string>
using namespace cnmfe;

template <class V> static void put(const char *name, const V &v) {
    std::printf("%s", name);
    for (auto x : v) std::printf(" %d", (int)x);
    std::printf("\n");
}
static std::vector<int> get(std::istream &in, size_t n) { std::vector<int> v(n); for (auto &x : v) in >> x; return v; }

int main(int argc, char **argv) {
    if (argc != 2) return 2;
    std::ifstream in(argv[1]);
    std::string cmd;
    while (in >> cmd) {
        if (cmd == "segments") {
            int n; in >> n;
            std::vector<int> out;
            for (int nb : get(in, n)) out.push_back(plan::win_segments(nb));
            put("nsg", out);
        } else if (cmd == "pairs") {
            int nr_b, nc_b, roff, coff, nr, nc, p; in >> nr_b >> nc_b >> roff >> coff >> nr >> nc >> p;
            const std::vector<int> dr = get(in, p), dc = get(in, p);
            const plan::Reach r = plan::ring_reach(dr.data(), dc.data(), p);
            put("reach", std::vector<int>{r.p_radius, r.maxd, r.nrel, r.nbw, r.woff, (int)r.ok});
            if (!r.ok) { std::printf("end\n"); continue; }
            put("count", std::vector<int>{plan::ring_pairs(nr_b, nc_b, roff, coff, nr, nc, r.p_radius, r.maxd, nullptr, nullptr)});      // (as bg_reserve asks)
            std::vector<plan::Pair> pairs; std::vector<int> pair_of, flat;
            const int n = plan::ring_pairs(nr_b, nc_b, roff, coff, nr, nc, r.p_radius, r.maxd, &pairs, &pair_of);
            if (n != (int)pairs.size()) return 3;
            for (const plan::Pair &q : pairs) { flat.push_back(q.a); flat.push_back(q.b); flat.push_back(q.rel); flat.push_back(q.pad); }
            plan::Tables t;
            plan::ring_tables(pairs, r.maxd, r.p_radius, dr.data(), dc.data(), p, t);
            put("pairs", flat); put("pair_of", pair_of); put("needmask", t.needmask); put("work", t.work); put("tcnt", t.tcnt); put("tlist", t.tlist);
        } else if (cmd == "lists") {
            int nr_b, nc_b, p_radius, K; in >> nr_b >> nc_b >> p_radius >> K;
            std::vector<int64_t> colptr(K + 1);
            for (auto &x : colptr) in >> x;
            const std::vector<int> rowidx = get(in, (size_t)colptr[K]);
            const int one[1] = {p_radius}, zero[1] = {0};
            const plan::Reach r = plan::ring_reach(one, zero, 1);
            const int nbr = (nr_b + 15) / 16, nbc = (nc_b + 15) / 16;
            std::vector<int> pair_blk, k_ptr, nbox, items, nmeta, lmeta;
            plan::footprint_blocks(K, colptr.data(), rowidx.data(), nr_b, nbr, nbc, r.maxd, pair_blk, k_ptr, nbox);
            plan::BlockLists L;
            const bool ok = plan::block_lists(nbr * nbc, K, pair_blk.data(), k_ptr.data(), L);
            put("maxd", std::vector<int>{r.maxd}); put("ok", std::vector<int>{(int)ok}); put("nbox", nbox);
            if (!ok) { std::printf("end\n"); continue; }
            plan::win_i8_items(L.blall, L.lst_ptr, items);
            put("lst_ptr", L.lst_ptr); put("lst_k", L.lst_k); put("slot_of", L.slot_of);
            put("nt0", L.blk_nt[0]); put("nt1", L.blk_nt[1]); put("nt2", L.blk_nt[2]); put("nt3", L.blk_nt[3]); put("blall", L.blall); put("items", items);
            put("stage", std::vector<long long>{(long long)plan::stage_windows(K, nbox, L.lst_k, nr_b, nc_b, p_radius, nmeta, lmeta)});
            put("nmeta", nmeta); put("lmeta", lmeta);
        } else return 4;
        std::printf("end\n");
    }
    return 0;
}
