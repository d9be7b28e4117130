// (g') the HOST rules of dsData (utilities/dsData.m:29-43) that ds.hpp's kernels and their callers share -- plain C++17, no device code, so that
// tests/ds_fold_driver.cpp builds them with the host compiler:
//   ds_box_taps   the tap table of imresize(., 'box') along one dimension (the separable `contributions` rule, mirrored border, normalised rows)
//   ds_fold_csc   A_ds: every column of a CSC footprint matrix on an nr x nc grid box-resized to ceil(nr / ssub) x ceil(nc / ssub) with those tables, in
//                 float64, as CSR (columns ascending within a row, exact zeros dropped).  dsData is linear, in space through the box resize and in time through
//                 the bin means, so dsData(Ysig - A C) = dsData(Ysig) - A_ds C_ds: the second pass (cnmfe_peel_open_residual_ds) subtracts the low-resolution
//                 product and no full-resolution difference video exists.
//   ds_bin_mean   C_ds: the mean of tsub consecutive samples, added in ascending order, ONE division (the rule of k_trace_bin_mean and of k_ds_video's bins)
#pragma once
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <vector>

#if defined(__HIPCC__)
#define DS_HD __host__ __device__ __forceinline__
#else
#define DS_HD inline
#endif

namespace cnmfe {

constexpr int DS_SSUB_MAX = 8;
constexpr int DS_NT_MAX = DS_SSUB_MAX + 1;            // non-zero box taps of one output sample: at most ceil(in / out) + 1 <= ssub + 1

// the non-zero taps of every output sample in ascending (virtual) order, padded to `nt` per sample with weight 0 on a valid index
struct DsTaps { int n_in = 0, n_out = 0, nt = 0; std::vector<int> idx; std::vector<double> w; };

static DsTaps ds_box_taps(int n_in, int n_out) {
    DsTaps t; t.n_in = n_in; t.n_out = n_out;
    const double scale = (double)n_out / (double)n_in;
    const double kw = scale < 1.0 ? 1.0 / scale : 1.0;
    const int P = (int)std::ceil(kw) + 2;
    std::vector<int> ii((size_t)n_out * P); std::vector<double> ww((size_t)n_out * P);
    std::vector<int> cnt((size_t)n_out, 0);
    for (int o = 0; o < n_out; ++o) {
        const double x = o + 1.0, u = x / scale + 0.5 * (1.0 - 1.0 / scale);
        const double left = std::floor(u - kw / 2);
        double sum = 0;
        int c = 0;
        for (int i = 0; i < P; ++i) {
            double d = u - (left + i);
            if (scale < 1.0) d = scale * d;
            if (!(d >= -0.5 && d < 0.5)) continue;
            const long v = (long)left + i - 1, per = 2L * n_in;   // 0-based virtual index, aux = [1:n n:-1:1]
            const long mth = ((v % per) + per) % per;
            ii[(size_t)o * P + c] = (int)(mth < n_in ? mth : per - 1 - mth); ww[(size_t)o * P + c] = 1.0; sum += 1.0; ++c;
        }
        for (int i = 0; i < c; ++i) ww[(size_t)o * P + i] /= sum;
        cnt[(size_t)o] = c; t.nt = std::max(t.nt, c);
    }
    t.idx.assign((size_t)n_out * t.nt, 0); t.w.assign((size_t)n_out * t.nt, 0.0);
    for (int o = 0; o < n_out; ++o)
        for (int i = 0; i < cnt[(size_t)o]; ++i) { t.idx[(size_t)o * t.nt + i] = ii[(size_t)o * P + i]; t.w[(size_t)o * t.nt + i] = ww[(size_t)o * P + i]; }
    return t;
}

// the mean of one bin: x[0 .. tsub) added in ascending order in fp64, divided once
template <typename T> DS_HD double ds_bin_mean(const T *x, int tsub) {
    double s = 0.0;
    for (int i = 0; i < tsub; ++i) s += (double)x[i];
    return s / (double)tsub;
}

// A_ds as the device takes it: CSR over the d1s * d2s low-resolution pixels (column-major), fp64 values
struct DsCSR { std::vector<int32_t> rowptr, col; std::vector<double> val; };

// A: nr * nc rows (column-major pixels) x K columns, CSC with float values.  Per column the taps of tr / tc are turned round (input sample -> the output samples
// it feeds; a mirrored sample appears once per tap), every stored entry is spread over its low-resolution cells, and the cells of the column's bounding box are
// emitted in ascending order.  false: more than 2^31 - 1 entries.
static bool ds_fold_csc(int nr, int nc, const DsTaps &tr, const DsTaps &tc, int32_t K, const int64_t *colptr, const int32_t *rowidx, const float *val, DsCSR &out) {
    const int d1s = tr.n_out, d2s = tc.n_out;
    const int64_t ds = (int64_t)d1s * d2s;
    // input sample -> (output sample, weight), output samples ascending
    auto turn = [](const DsTaps &t, std::vector<int> &first, std::vector<int> &o_of, std::vector<double> &w_of) {
        first.assign((size_t)t.n_in + 1, 0);
        for (int o = 0; o < t.n_out; ++o)
            for (int k = 0; k < t.nt; ++k) if (t.w[(size_t)o * t.nt + k] != 0.0) first[(size_t)t.idx[(size_t)o * t.nt + k] + 1]++;
        for (int i = 0; i < t.n_in; ++i) first[(size_t)i + 1] += first[(size_t)i];
        o_of.resize((size_t)first[(size_t)t.n_in]); w_of.resize(o_of.size());
        std::vector<int> cur(first.begin(), first.end() - 1);
        for (int o = 0; o < t.n_out; ++o)
            for (int k = 0; k < t.nt; ++k) {
                const double w = t.w[(size_t)o * t.nt + k];
                if (w == 0.0) continue;
                const int pos = cur[(size_t)t.idx[(size_t)o * t.nt + k]]++;
                o_of[(size_t)pos] = o; w_of[(size_t)pos] = w;
            }
    };
    std::vector<int> fr, fc, orow, ocol; std::vector<double> wrow, wcol;
    turn(tr, fr, orow, wrow); turn(tc, fc, ocol, wcol);
    std::vector<double> img((size_t)ds, 0.0);
    std::vector<int32_t> crow, ccol; std::vector<double> cval;             // the entries column by column
    (void)nc;
    for (int32_t k = 0; k < K; ++k) {
        int r_lo = d1s, r_hi = -1, c_lo = d2s, c_hi = -1;                    // the column's bounding box on the low-resolution grid
        for (int64_t e = colptr[k]; e < colptr[k + 1]; ++e) {
            const int r = (int)(rowidx[e] % nr), c = (int)(rowidx[e] / nr);
            const double a = (double)val[e];
            for (int jc = fc[(size_t)c]; jc < fc[(size_t)c + 1]; ++jc)
                for (int jr = fr[(size_t)r]; jr < fr[(size_t)r + 1]; ++jr) {
                    const int oc = ocol[(size_t)jc], orr = orow[(size_t)jr];
                    img[(size_t)oc * d1s + orr] += wcol[(size_t)jc] * wrow[(size_t)jr] * a;
                    r_lo = std::min(r_lo, orr); r_hi = std::max(r_hi, orr); c_lo = std::min(c_lo, oc); c_hi = std::max(c_hi, oc);
                }
        }
        for (int oc = c_lo; oc <= c_hi; ++oc)
            for (int orr = r_lo; orr <= r_hi; ++orr) {
                double &v = img[(size_t)oc * d1s + orr];
                if (v != 0.0) { crow.push_back((int32_t)(oc * d1s + orr)); ccol.push_back(k); cval.push_back(v); }
                v = 0.0;
            }
        if (crow.size() > (size_t)INT32_MAX) return false;
    }
    const size_t nnz = crow.size();
    out.rowptr.assign((size_t)ds + 1, 0); out.col.resize(nnz); out.val.resize(nnz);
    for (size_t e = 0; e < nnz; ++e) out.rowptr[(size_t)crow[e] + 1]++;
    for (int64_t p = 0; p < ds; ++p) out.rowptr[(size_t)p + 1] += out.rowptr[(size_t)p];
    std::vector<int32_t> cur(out.rowptr.begin(), out.rowptr.end() - 1);
    for (size_t e = 0; e < nnz; ++e) {                                        // (columns were visited in ascending order: ascending within every row)
        const int32_t pos = cur[(size_t)crow[e]]++;
        out.col[(size_t)pos] = ccol[e]; out.val[(size_t)pos] = cval[e];
    }
    return true;
}

}  // namespace cnmfe
