// TEST INFRASTRUCTURE: cnmf_e_amd/csrc/ds_fold.hpp -- the host rules of the down-sampled second pass (the box tap tables, A_ds, the bin mean) -- built with the
// host compiler and the address / undefined-behaviour sanitizers, driven by tests/test_residual_ds_oracle.py.
//   ds_fold_driver IN OUT
// IN  (little-endian): int32 nr, nc, ssub, tsub, K, T | int64 colptr[K + 1] | int32 rowidx[nnz] | float val[nnz] | float C[K * T] (row-major)
// OUT: int32 d1s, d2s, Ts, nnz_ds | int32 rowptr[d1s d2s + 1] | int32 col[nnz_ds] | double val[nnz_ds] | double C_ds[K * Ts]
#include "../cnmf_e_amd/csrc/ds_fold.hpp"
#include <cstdio>
#include <cstdlib>
#include <vector>

template <class T> static void rd(FILE *f, T *p, size_t n) { if (n && fread(p, sizeof(T), n, f) != n) { fprintf(stderr, "short read\n"); exit(2); } }
template <class T> static void wr(FILE *f, const T *p, size_t n) { if (n && fwrite(p, sizeof(T), n, f) != n) { fprintf(stderr, "short write\n"); exit(2); } }

int main(int argc, char **argv) {
    if (argc != 3) { fprintf(stderr, "usage: ds_fold_driver IN OUT\n"); return 2; }
    FILE *in = fopen(argv[1], "rb");
    if (!in) { perror(argv[1]); return 2; }
    int32_t h[6];
    rd(in, h, 6);
    const int nr = h[0], nc = h[1], ssub = h[2], tsub = h[3], K = h[4], T = h[5];
    std::vector<int64_t> colptr((size_t)K + 1);
    rd(in, colptr.data(), colptr.size());
    const size_t nnz = (size_t)colptr[(size_t)K];
    std::vector<int32_t> rowidx(nnz); std::vector<float> val(nnz), C((size_t)K * T);
    rd(in, rowidx.data(), nnz); rd(in, val.data(), nnz); rd(in, C.data(), C.size());
    fclose(in);

    const int d1s = (nr + ssub - 1) / ssub, d2s = (nc + ssub - 1) / ssub, Ts = T / tsub;
    const cnmfe::DsTaps tr = cnmfe::ds_box_taps(nr, d1s), tc = cnmfe::ds_box_taps(nc, d2s);
    if (tr.nt > cnmfe::DS_NT_MAX || tc.nt > cnmfe::DS_NT_MAX) { fprintf(stderr, "%d / %d taps\n", tr.nt, tc.nt); return 3; }
    cnmfe::DsCSR a;
    if (!cnmfe::ds_fold_csc(nr, nc, tr, tc, K, colptr.data(), rowidx.data(), val.data(), a)) { fprintf(stderr, "too many entries\n"); return 3; }
    // the contract of the CSR the kernel walks: columns ascending within a row, no exact zero stored
    for (int64_t p = 0; p < (int64_t)d1s * d2s; ++p)
        for (int32_t e = a.rowptr[(size_t)p]; e < a.rowptr[(size_t)p + 1]; ++e) {
            if (a.val[(size_t)e] == 0.0) { fprintf(stderr, "a zero is stored in row %lld\n", (long long)p); return 4; }
            if (e > a.rowptr[(size_t)p] && a.col[(size_t)e - 1] >= a.col[(size_t)e]) { fprintf(stderr, "columns of row %lld do not ascend\n", (long long)p); return 4; }
        }
    std::vector<double> cds((size_t)K * Ts);
    for (int k = 0; k < K; ++k)
        for (int t = 0; t < Ts; ++t) cds[(size_t)k * Ts + t] = cnmfe::ds_bin_mean(C.data() + (size_t)k * T + (size_t)t * tsub, tsub);

    FILE *out = fopen(argv[2], "wb");
    if (!out) { perror(argv[2]); return 2; }
    const int32_t o[4] = {d1s, d2s, Ts, (int32_t)a.col.size()};
    wr(out, o, 4); wr(out, a.rowptr.data(), a.rowptr.size()); wr(out, a.col.data(), a.col.size()); wr(out, a.val.data(), a.val.size()); wr(out, cds.data(), cds.size());
    fclose(out);
    return 0;
}
