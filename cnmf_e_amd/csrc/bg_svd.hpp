// background_model = 'svd' (fit_svd_model.m / svdsecon.m of the reference): the top-nb singular triplets of the block's background residual
//     X = Yc - A Cc - r 1'        (d_b x T;  Yc the resident centred video, Cc the centred traces, r = mean(Yc - A Cc, 2))
// WITHOUT forming X, X X' or X' X: block subspace iteration with a Rayleigh-Ritz step on a panel of SVQ = 16 columns (nb <= 8: at least 8 guard columns).
// One iteration is two reads of the video:
//     G = X' Q   (T x 16)    k_svd_project: a reduction over PIXELS; 128-pixel x 64-frame tiles through LDS, fp64 sums, pixel segments added in fixed order
//     Z = X G    (d_b x 16)  k_svd_expand:  a reduction over FRAMES; one lane per pixel streams its float4 frame groups, the G rows of a frame segment sit in LDS,
//                                           sixteen fp64 sums in registers, frame segments added in fixed order
// The footprint and the mean parts of X enter through small fp64 kernels (A'Q, Cc G, r'Q, 1'G) in the two "finish" kernels; a bound C never comes down.
// H = G'G = Q' (X X') Q is the Ritz problem (16 x 16, solved on the host in float64 by cyclic Jacobi); the panel is rotated by its eigenvectors, so column i converges
// to the i-th singular vector; the residual |M q_i - theta_i q_i|, M = X X', is MEASURED (k_svd_axpy + the panel Gram), not derived from the Ritz values; the next
// panel is Z V orthonormalised by CholeskyQR applied twice (panel Gram on the device in fixed order, the 16 x 16 factor on the host).
// No floating-point atomics anywhere: two fits of the same input give the same bits.
// k_lowrank_resid writes the background-subtracted patch Ysig = Yc + (Ymean - b0) - b f (fp64, ONE rounding to fp32): one read of the block video, one write of the patch.
// thresh_outlier and sn are dead for this model: fit_svd_model.m:29 tests a misspelt variable, its outlier branch never runs.  They stay dead here.
#pragma once
#include "common.hpp"

namespace cnmfe {

constexpr int SVQ = 16;                 // panel width: one N tile of v_mfma_f64_16x16x4_f64, and 8 guard columns beside the largest nb
constexpr int SVD_NB_MAX = 8;
constexpr int SVD_GRAM_ROWS = 1024;     // rows of a panel one workgroup of k_svd_gram / k_svd_colsum sums

// the start panel: a counter hash of (pixel, column) -- splitmix64 of the pair, mapped to (-1, 1); no library generator, the same on every run and every device
__global__ void k_svd_start(double *__restrict__ Q, int64_t n, int qe) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n * SVQ) return;
    const int j = (int)(i & 15);
    uint64_t z = (uint64_t)(i >> 4) * 0x9E3779B97F4A7C15ull + (uint64_t)(j + 1) * 0xD1B54A32D192ED03ull;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull; z = (z ^ (z >> 27)) * 0x94D049BB133111EBull; z ^= z >> 31;
    Q[i] = j < qe ? (double)(z >> 11) * (2.0 / 9007199254740992.0) - 1.0 : 0.0;
}

// rowsum[q] = sum_t Yc(q, t) in fp64, frames in order (the tail lanes of the last frame group hold zeros)
__global__ void k_svd_rowsum(const float4 *__restrict__ Yc4, int64_t d_b, int64_t Tc, double *__restrict__ rs) {
    const int64_t q = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (q >= d_b) return;
    double s0 = 0, s1 = 0, s2 = 0, s3 = 0;
    for (int64_t c = 0; c < Tc; ++c) { const float4 v = Yc4[c * d_b + q]; s0 += v.x; s1 += v.y; s2 += v.z; s3 += v.w; }
    rs[q] = (s0 + s1) + (s2 + s3);
}
// csum[k] = sum_t Cc(k, t): what the fp32 storage of the centred traces leaves of their mean
__global__ void k_svd_csum(const float *__restrict__ Cc, int64_t ldc, int64_t T, double *__restrict__ csum) {
    __shared__ double red[256];
    const float *row = Cc + (int64_t)blockIdx.x * ldc;
    double s = 0;
    for (int64_t t = threadIdx.x; t < T; t += 256) s += row[t];
    red[threadIdx.x] = s;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) { if ((int)threadIdx.x < o) red[threadIdx.x] += red[threadIdx.x + o]; __syncthreads(); }
    if (threadIdx.x == 0) csum[blockIdx.x] = red[0];
}
// r[q] = (rowsum[q] - sum_k A(q, k) csum[k]) / T  (A: CSR over the block rows; rowptr == nullptr: no footprints)
__global__ void k_svd_rmean(const double *__restrict__ rs, const int *__restrict__ rowptr, const int *__restrict__ col, const float *__restrict__ val,
                            const double *__restrict__ csum, int64_t d_b, int64_t T, double *__restrict__ r) {
    const int64_t q = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (q >= d_b) return;
    double a = 0;
    if (rowptr) for (int e = rowptr[q]; e < rowptr[q + 1]; ++e) a += (double)val[e] * csum[col[e]];
    r[q] = (rs[q] - a) / (double)T;
}

// ---- G = X' Q: the reduction over pixels ----------------------------------------------------------------------------------------------------------------------------
// A workgroup owns 64 frames (16 frame groups) and one pixel segment.  Per 128-pixel tile it stages the video as Ys[group][pixel] (float4: coalesced 16-byte loads,
// one pixel per lane) and the panel rows as Qs[pixel][column]; thread (half h, group g, column pair jp) adds the products of its half of the tile's pixels, in pixel
// order, into 4 frames x 2 columns of fp64 registers: one 16-byte LDS read of the video and one of the panel per 8 multiply-adds.  The two halves are added at the
// end (half 0 + half 1): every sum has one fixed order.  part[seg][Tpad][16]; 8 B of panel are read per 16 B of video.
__global__ __launch_bounds__(256) void k_svd_project(const float4 *__restrict__ Yc4, int64_t d_b, int64_t Tc, const double *__restrict__ Q, int64_t pseg,
                                                     double *__restrict__ part, int64_t Tpad) {
    __shared__ float4 Ys[16][129];                                // (a row of 129: the sixteen frame groups a wave reads at one pixel fall on sixteen different bank quads)
    __shared__ double Qs[128][SVQ];
    const int tid = threadIdx.x, jp = tid & 7, g = (tid >> 3) & 15, h = tid >> 7;
    const int64_t c0 = (int64_t)blockIdx.x * 16;
    const int64_t p0 = (int64_t)blockIdx.y * pseg, p1 = p0 + pseg < d_b ? p0 + pseg : d_b;
    double a[4][2] = {{0, 0}, {0, 0}, {0, 0}, {0, 0}};
    for (int64_t pt = p0; pt < p1; pt += 128) {
        const int lp = tid & 127;
#pragma unroll
        for (int r = 0; r < 8; ++r) {
            const int gg = h + 2 * r;
            float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
            if (pt + lp < p1 && c0 + gg < Tc) v = Yc4[(c0 + gg) * d_b + pt + lp];
            Ys[gg][lp] = v;
        }
#pragma unroll
        for (int r = 0; r < 8; ++r) {
            const int i = tid + 256 * r;                          // element of the 128 x 16 tile: row i >> 4, column i & 15
            (&Qs[0][0])[i] = pt + (i >> 4) < p1 ? Q[pt * SVQ + i] : 0.0;
        }
        __syncthreads();
        const int pb = h * 64;
#pragma unroll 4
        for (int pp = pb; pp < pb + 64; ++pp) {
            const float4 y = Ys[g][pp];
            const double q0 = Qs[pp][2 * jp], q1 = Qs[pp][2 * jp + 1];
            a[0][0] += (double)y.x * q0; a[0][1] += (double)y.x * q1;
            a[1][0] += (double)y.y * q0; a[1][1] += (double)y.y * q1;
            a[2][0] += (double)y.z * q0; a[2][1] += (double)y.z * q1;
            a[3][0] += (double)y.w * q0; a[3][1] += (double)y.w * q1;
        }
        __syncthreads();
    }
    double *red = &Qs[0][0];                                      // (free behind the loop's last barrier: 128 x 8 of its 2048 doubles)
    if (h == 1) {
#pragma unroll
        for (int k = 0; k < 8; ++k) red[(tid & 127) * 8 + k] = a[k >> 1][k & 1];
    }
    __syncthreads();
    if (h == 0) {
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            const int64_t t = (c0 + g) * 4 + (k >> 1);
            part[((int64_t)blockIdx.y * Tpad + t) * SVQ + 2 * jp + (k & 1)] = a[k >> 1][k & 1] + red[tid * 8 + k];
        }
    }
}
// G(t, j) = sum_seg part - sum_k Cc(k, t) (A'Q)(k, j) - (r'Q)(j)
__global__ void k_svd_g_finish(const double *__restrict__ part, int nseg, int64_t Tpad, int64_t T, const float *__restrict__ Cc, int64_t ldc, int K,
                               const double *__restrict__ AtQ, const double *__restrict__ rq, double *__restrict__ G) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= T * SVQ) return;
    const int64_t t = i >> 4; const int j = (int)(i & 15);
    double s = 0;
    for (int sg = 0; sg < nseg; ++sg) s += part[((int64_t)sg * Tpad + t) * SVQ + j];
    double c = 0;
    for (int k = 0; k < K; ++k) c += (double)Cc[(int64_t)k * ldc + t] * AtQ[k * SVQ + j];
    G[i] = s - c - rq[j];
}

// ---- Z = X G: the reduction over frames -----------------------------------------------------------------------------------------------------------------------------
// One lane per pixel, one frame segment per workgroup row.  The G rows of 64 frames (8 KB) are staged in LDS; the lane streams its float4 frame groups, four 16-byte
// loads in flight, and adds into sixteen fp64 registers in frame order.  The LDS reads are wave-uniform (broadcast).  part[seg][d_b][16].
__global__ __launch_bounds__(256) void k_svd_expand(const float4 *__restrict__ Yc4, int64_t d_b, int64_t Tc, int64_t T, const double *__restrict__ G, int64_t cseg,
                                                    double *__restrict__ part) {
    __shared__ double Gs[64][SVQ];
    const int tid = threadIdx.x;
    const int64_t p = (int64_t)blockIdx.x * 256 + tid;
    const int64_t c0 = (int64_t)blockIdx.y * cseg, c1 = c0 + cseg < Tc ? c0 + cseg : Tc;
    double acc[SVQ];
#pragma unroll
    for (int j = 0; j < SVQ; ++j) acc[j] = 0;
    for (int64_t cb = c0; cb < c1; cb += 16) {
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int i = tid + 256 * r;
            const int64_t t = cb * 4 + (i >> 4);
            (&Gs[0][0])[i] = t < T ? G[t * SVQ + (i & 15)] : 0.0;
        }
        __syncthreads();
        const int nc = (int)(c1 - cb < 16 ? c1 - cb : 16);
        for (int cc = 0; cc < nc; cc += 4) {
            float4 v[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                v[u] = make_float4(0.f, 0.f, 0.f, 0.f);
                if (p < d_b && cc + u < nc) v[u] = Yc4[(cb + cc + u) * d_b + p];
            }
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const double y0 = v[u].x, y1 = v[u].y, y2 = v[u].z, y3 = v[u].w;
                const int row = (cc + u) * 4;
#pragma unroll
                for (int j = 0; j < SVQ; ++j) {
                    acc[j] += y0 * Gs[row][j]; acc[j] += y1 * Gs[row + 1][j]; acc[j] += y2 * Gs[row + 2][j]; acc[j] += y3 * Gs[row + 3][j];
                }
            }
        }
        __syncthreads();
    }
    if (p < d_b) {
        double *o = part + ((int64_t)blockIdx.y * d_b + p) * SVQ;
#pragma unroll
        for (int j = 0; j < SVQ; ++j) o[j] = acc[j];
    }
}
// Z(q, j) = sum_seg part - sum_k A(q, k) (Cc G)(k, j) - r(q) (1'G)(j)
__global__ void k_svd_z_finish(const double *__restrict__ part, int nseg, int64_t d_b, const int *__restrict__ rowptr, const int *__restrict__ col,
                               const float *__restrict__ val, const double *__restrict__ CG, const double *__restrict__ r, const double *__restrict__ sumG,
                               double *__restrict__ Z) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= d_b * SVQ) return;
    const int64_t q = i >> 4; const int j = (int)(i & 15);
    double s = 0;
    for (int sg = 0; sg < nseg; ++sg) s += part[((int64_t)sg * d_b + q) * SVQ + j];
    double a = 0;
    if (rowptr) for (int e = rowptr[q]; e < rowptr[q + 1]; ++e) a += (double)val[e] * CG[col[e] * SVQ + j];
    Z[i] = s - a - r[q] * sumG[j];
}

// ---- the small fp64 products ------------------------------------------------------------------------------------------------------------------------------------------
// out(k, j) = sum_e val[e] W(rowidx[e], j) over CSC column k (A'Q); one workgroup per column, sixteen row lanes per panel column, added in lane order
__global__ __launch_bounds__(256) void k_svd_atq(const int64_t *__restrict__ colptr, const int *__restrict__ rowidx, const float *__restrict__ val,
                                                 const double *__restrict__ W, double *__restrict__ out) {
    __shared__ double red[16][SVQ];
    const int j = threadIdx.x & 15, l = threadIdx.x >> 4, k = blockIdx.x;
    double s = 0;
    for (int64_t e = colptr[k] + l; e < colptr[k + 1]; e += 16) s += (double)val[e] * W[(int64_t)rowidx[e] * SVQ + j];
    red[l][j] = s;
    __syncthreads();
    if (l == 0) { double t = 0; for (int i = 0; i < 16; ++i) t += red[i][j]; out[k * SVQ + j] = t; }
}
// out(k, j) = sum_t Cc(k, t) G(t, j)
__global__ __launch_bounds__(256) void k_svd_cg(const float *__restrict__ Cc, int64_t ldc, int64_t T, const double *__restrict__ G, double *__restrict__ out) {
    __shared__ double red[16][SVQ];
    const int j = threadIdx.x & 15, l = threadIdx.x >> 4, k = blockIdx.x;
    const float *row = Cc + (int64_t)k * ldc;
    double s = 0;
    for (int64_t t = l; t < T; t += 16) s += (double)row[t] * G[t * SVQ + j];
    red[l][j] = s;
    __syncthreads();
    if (l == 0) { double t = 0; for (int i = 0; i < 16; ++i) t += red[i][j]; out[k * SVQ + j] = t; }
}
// part[blk][j] = sum over the block's rows of w(row) W(row, j)   (w == nullptr: ones)
__global__ __launch_bounds__(256) void k_svd_colsum(const double *__restrict__ W, const double *__restrict__ w, int64_t n, double *__restrict__ part) {
    __shared__ double red[16][SVQ];
    const int j = threadIdx.x & 15, l = threadIdx.x >> 4;
    const int64_t r0 = (int64_t)blockIdx.x * SVD_GRAM_ROWS, r1 = r0 + SVD_GRAM_ROWS < n ? r0 + SVD_GRAM_ROWS : n;
    double s = 0;
    for (int64_t r = r0 + l; r < r1; r += 16) s += (w ? w[r] : 1.0) * W[r * SVQ + j];
    red[l][j] = s;
    __syncthreads();
    if (l == 0) { double t = 0; for (int i = 0; i < 16; ++i) t += red[i][j]; part[(int64_t)blockIdx.x * SVQ + j] = t; }
}
// part[blk][i][j] = sum over the block's rows of Wa(row, i) Wb(row, j), rows in order
__global__ __launch_bounds__(256) void k_svd_gram(const double *__restrict__ Wa, const double *__restrict__ Wb, int64_t n, double *__restrict__ part) {
    const int j = threadIdx.x & 15, i = threadIdx.x >> 4;
    const int64_t r0 = (int64_t)blockIdx.x * SVD_GRAM_ROWS, r1 = r0 + SVD_GRAM_ROWS < n ? r0 + SVD_GRAM_ROWS : n;
    double s = 0;
#pragma unroll 8
    for (int64_t r = r0; r < r1; ++r) s += Wa[r * SVQ + i] * Wb[r * SVQ + j];
    part[(int64_t)blockIdx.x * 256 + threadIdx.x] = s;
}
// out[i] = sum_b part[b][i], b in order (m values per part)
__global__ void k_svd_reduce(const double *__restrict__ part, int nparts, int m, double *__restrict__ out) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= m) return;
    double s = 0;
    for (int b = 0; b < nparts; ++b) s += part[(int64_t)b * m + i];
    out[i] = s;
}
// W <- W M (n x 16 by 16 x 16, in place: a lane owns a row)
__global__ __launch_bounds__(256) void k_svd_mul16(double *__restrict__ W, int64_t n, const double *__restrict__ M) {
    __shared__ double Ms[SVQ][SVQ];
    (&Ms[0][0])[threadIdx.x] = M[threadIdx.x];
    __syncthreads();
    const int64_t r = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (r >= n) return;
    double w[SVQ], o[SVQ];
#pragma unroll
    for (int i = 0; i < SVQ; ++i) w[i] = W[r * SVQ + i];
#pragma unroll
    for (int j = 0; j < SVQ; ++j) {
        double s = 0;
#pragma unroll
        for (int i = 0; i < SVQ; ++i) s += w[i] * Ms[i][j];
        o[j] = s;
    }
#pragma unroll
    for (int j = 0; j < SVQ; ++j) W[r * SVQ + j] = o[j];
}
// D = Z - Q diag(theta): the columns whose norms are the residuals of the Ritz pairs
__global__ void k_svd_axpy(const double *__restrict__ Z, const double *__restrict__ Q, const double *__restrict__ theta, int64_t n, double *__restrict__ D) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n * SVQ) return;
    D[i] = Z[i] - theta[i & 15] * Q[i];
}
// sign[j] = -1 where the entry of largest magnitude of column j is negative (the first such entry on ties), else +1
__global__ __launch_bounds__(256) void k_svd_sign(const double *__restrict__ Q, int64_t n, double *__restrict__ sign) {
    __shared__ double bv[256]; __shared__ long long bi[256];
    const int j = blockIdx.x;
    double best = 0; long long idx = -1;
    for (int64_t r = threadIdx.x; r < n; r += 256) { const double v = Q[r * SVQ + j]; if (idx < 0 || fabs(v) > fabs(best)) { best = v; idx = r; } }
    bv[threadIdx.x] = best; bi[threadIdx.x] = idx;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if ((int)threadIdx.x < o) {
            const double v = bv[threadIdx.x + o]; const long long k = bi[threadIdx.x + o];
            const double m = bv[threadIdx.x]; const long long km = bi[threadIdx.x];
            if (k >= 0 && (km < 0 || fabs(v) > fabs(m) || (fabs(v) == fabs(m) && k < km))) { bv[threadIdx.x] = v; bi[threadIdx.x] = k; }
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) sign[j] = bv[0] < 0 ? -1.0 : 1.0;
}

// ---- the factors of the patch -----------------------------------------------------------------------------------------------------------------------------------------
// fin: [0..15] s, [16..31] sign, [32..47] 1'G of the rotated panel
// f(i, t) = sign_i G(t, i) / s_i   (s_i = 0: a zero row, never a NaN)
__global__ void k_svd_f(const double *__restrict__ G, int64_t T, int nb, const double *__restrict__ fin, double *__restrict__ f) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= T * nb) return;
    const int c = (int)(i / T); const int64_t t = i % T;
    const double s = fin[c];
    f[i] = s > 0 ? fin[16 + c] * G[t * SVQ + c] / s : 0.0;
}
// b(m, i) = sign_i u(q(m), i) s_i on the patch pixels, b0(m) = Ymean(q) - A(q, :) Cmean - b(m, :) mean(f, 2)
__global__ void k_svd_b(const double *__restrict__ Q, int nb, const double *__restrict__ fin, const double *__restrict__ ymean, const int *__restrict__ rowptr,
                        const int *__restrict__ col, const float *__restrict__ val, const double *__restrict__ Cm, int64_t d, int64_t T, int nr, int nr_b, int roff,
                        int coff, double *__restrict__ b, double *__restrict__ b0) {
    const int64_t m = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (m >= d) return;
    const int64_t q = (int64_t)((int)(m / nr) + coff) * nr_b + (int)(m % nr) + roff;
    double a = 0;
    if (rowptr) for (int e = rowptr[q]; e < rowptr[q + 1]; ++e) a += (double)val[e] * Cm[col[e]];
    double bm = 0;
    for (int i = 0; i < nb; ++i) {
        const double s = fin[i], sg = fin[16 + i];
        const double bi = sg * Q[q * SVQ + i] * s;
        b[(int64_t)i * d + m] = bi;
        bm += bi * (s > 0 ? sg * fin[32 + i] / (s * (double)T) : 0.0);
    }
    b0[m] = ymean[q] - a - bm;
}

// Ysig(m, t) = Yc(q, t) + (ymean_f(q) - b0(m)) - sum_i b(m, i) f(i, t): fp64, one rounding to fp32.  Yc was centred about the fp32 mean (k_center4), so that is
// the mean that comes back.  The lanes of the last frame group beyond T hold zeros, as in every Ysig4.
__global__ __launch_bounds__(256) void k_lowrank_resid(const float4 *__restrict__ Yc4, const float *__restrict__ ymean_f, const double *__restrict__ b0,
                                                       const double *__restrict__ b, const double *__restrict__ f, int nb, int64_t d, int64_t d_b, int64_t T, int nr,
                                                       int nr_b, int roff, int coff, float4 *__restrict__ out) {
    const int64_t m = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (m >= d) return;
    const int64_t c = blockIdx.y, t = 4 * c;
    const int64_t q = (int64_t)((int)(m / nr) + coff) * nr_b + (int)(m % nr) + roff;
    const float4 y = Yc4[c * d_b + q];
    const double dl = (double)ymean_f[q] - b0[m];
    double bf0 = 0, bf1 = 0, bf2 = 0, bf3 = 0;
    for (int i = 0; i < nb; ++i) {
        const double bi = b[(int64_t)i * d + m];
        const double *fr = f + (int64_t)i * T + t;
        bf0 += bi * fr[0];
        if (t + 1 < T) bf1 += bi * fr[1];
        if (t + 2 < T) bf2 += bi * fr[2];
        if (t + 3 < T) bf3 += bi * fr[3];
    }
    float4 o;
    o.x = (float)(((double)y.x + dl) - bf0);
    o.y = t + 1 < T ? (float)(((double)y.y + dl) - bf1) : 0.f;
    o.z = t + 2 < T ? (float)(((double)y.z + dl) - bf2) : 0.f;
    o.w = t + 3 < T ? (float)(((double)y.w + dl) - bf3) : 0.f;
    out[c * d + m] = o;
}

// ---- host: the 16 x 16 problems in float64 ----------------------------------------------------------------------------------------------------------------------------
// eigenpairs of a symmetric 16 x 16 matrix by cyclic Jacobi, eigenvalues descending; V columns are the vectors (row-major V[i][j])
inline void svd_eigh16(const double *H, double *theta, double *V) {
    const int n = SVQ;
    double A[SVQ][SVQ], E[SVQ][SVQ];
    for (int i = 0; i < n; ++i) for (int j = 0; j < n; ++j) { A[i][j] = 0.5 * (H[i * n + j] + H[j * n + i]); E[i][j] = i == j; }
    for (int sweep = 0; sweep < 60; ++sweep) {
        double off = 0, dia = 0;
        for (int i = 0; i < n; ++i) for (int j = 0; j < n; ++j) (i == j ? dia : off) += A[i][j] * A[i][j];
        if (off <= 1e-40 * dia || off == 0) break;
        for (int p = 0; p < n - 1; ++p) for (int q = p + 1; q < n; ++q) {
            if (A[p][q] == 0) continue;
            const double tau = (A[q][q] - A[p][p]) / (2 * A[p][q]);
            const double t = (tau >= 0 ? 1.0 : -1.0) / (std::fabs(tau) + std::sqrt(1 + tau * tau));
            const double c = 1 / std::sqrt(1 + t * t), s = t * c;
            for (int k = 0; k < n; ++k) { const double x = A[k][p], y = A[k][q]; A[k][p] = c * x - s * y; A[k][q] = s * x + c * y; }
            for (int k = 0; k < n; ++k) { const double x = A[p][k], y = A[q][k]; A[p][k] = c * x - s * y; A[q][k] = s * x + c * y; }
            for (int k = 0; k < n; ++k) { const double x = E[k][p], y = E[k][q]; E[k][p] = c * x - s * y; E[k][q] = s * x + c * y; }
        }
    }
    int ord[SVQ];
    for (int i = 0; i < n; ++i) ord[i] = i;
    std::stable_sort(ord, ord + n, [&](int a, int b) { return A[a][a] > A[b][b]; });
    for (int j = 0; j < n; ++j) { theta[j] = A[ord[j]][ord[j]]; for (int i = 0; i < n; ++i) V[i * n + j] = E[i][ord[j]]; }
}
// S = R'R (upper R), Rinv = inv(R) so that W Rinv has orthonormal columns.  A column that has no component outside the span of those before it (a pivot
// at rounding level: a panel wider than the rank of X) is dropped -- its column of Rinv is zero, the panel column becomes zero and stays so.
inline void svd_chol_inv16(const double *S, double *Rinv) {
    const int n = SVQ;
    double R[SVQ][SVQ] = {}; bool dead[SVQ] = {};
    double dmax = 0;
    for (int i = 0; i < n; ++i) dmax = std::max(dmax, S[i * n + i]);
    for (int j = 0; j < n; ++j) {
        for (int i = 0; i < j; ++i) {
            double s = S[i * n + j];
            for (int k = 0; k < i; ++k) s -= R[k][i] * R[k][j];
            R[i][j] = dead[i] ? 0.0 : s / R[i][i];
        }
        double p = S[j * n + j];
        for (int k = 0; k < j; ++k) p -= R[k][j] * R[k][j];
        if (!(p > 1e-24 * dmax) || !(p > 0)) { dead[j] = true; R[j][j] = 1.0; for (int i = 0; i < j; ++i) R[i][j] = 0.0; }
        else R[j][j] = std::sqrt(p);
    }
    for (int j = 0; j < n; ++j) {                                   // back substitution, column by column: R Rinv = I
        for (int i = n - 1; i >= 0; --i) {
            double s = i == j ? 1.0 : 0.0;
            for (int k = i + 1; k <= j; ++k) s -= R[i][k] * Rinv[k * n + j];
            Rinv[i * n + j] = i > j ? 0.0 : s / R[i][i];
        }
        if (dead[j]) for (int i = 0; i < n; ++i) Rinv[i * n + j] = 0.0;
    }
}

// ---- host: the fit ------------------------------------------------------------------------------------------------------------------------------------------------------
struct SvdWork { cnmfe_ctx *ctx; Patch *P; int K; int64_t ldc; const float *Cc; const int64_t *colptr; const int *rowidx; const float *cval; const int *rowptr, *rcol; const float *rval; };
// scratch of a fit in LaneState::svd: [0] Q, [1] Z, [2] G, [3] D, [4] part, [5] A'Q, [6] Cc G, [7] r, [8] rowsum | csum, [9] small (rq | sumG | theta | M | fin), [10] Gram out,
// [11..13] A as CSC, [14..16] A as CSR, [17] a 16 x 16 factor on its way to k_svd_mul16, [18] theta
enum { SV_Q = 0, SV_Z, SV_G, SV_D, SV_PART, SV_ATQ, SV_CG, SV_R, SV_RS, SV_SMALL, SV_GRAM, SV_CP, SV_RI, SV_CV, SV_RP, SV_RC, SV_RV, SV_M, SV_TH, SV_N };
static int svd_colsum(SvdWork &w, const double *W, const double *wt, int64_t n, double *out16) {
    cnmfe_ctx *ctx = w.ctx;
    const int nblk = (int)((n + SVD_GRAM_ROWS - 1) / SVD_GRAM_ROWS);
    double *part = ctx->svd[SV_PART].as<double>();
    LAUNCH(ctx, "svd_colsum", k_svd_colsum, dim3(nblk), dim3(256), 0, W, wt, n, part);
    LAUNCH(ctx, "svd_reduce", k_svd_reduce, dim3(1), dim3(256), 0, part, nblk, SVQ, out16);
    return 0;
}
static int svd_gram(SvdWork &w, const double *Wa, const double *Wb, int64_t n, double *host256) {
    cnmfe_ctx *ctx = w.ctx;
    const int nblk = (int)((n + SVD_GRAM_ROWS - 1) / SVD_GRAM_ROWS);
    double *part = ctx->svd[SV_PART].as<double>(), *out = ctx->svd[SV_GRAM].as<double>();
    LAUNCH(ctx, "svd_gram", k_svd_gram, dim3(nblk), dim3(256), 0, Wa, Wb, n, part);
    LAUNCH(ctx, "svd_reduce", k_svd_reduce, dim3(1), dim3(256), 0, part, nblk, 256, out);
    CK(hipMemcpyAsync(host256, out, 256 * sizeof(double), hipMemcpyDeviceToHost, ctx->st()));
    CK(hipStreamSynchronize(ctx->st()));
    return 0;
}
static int svd_mul(SvdWork &w, double *W, int64_t n, const double *M_host) {
    cnmfe_ctx *ctx = w.ctx;
    RET(to_dev(ctx, ctx->svd[SV_M], M_host, 256));               // (staged in the pinned arena: M_host, the caller's stack, is free at once and nothing waits)
    LAUNCH(ctx, "svd_mul16", k_svd_mul16, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, W, n, ctx->svd[SV_M].as<double>());
    return 0;
}
// W <- orth(W) by CholeskyQR, twice
static int svd_orth(SvdWork &w, double *W, int64_t n) {
    for (int pass = 0; pass < 2; ++pass) {
        double S[256], Rinv[256];
        RET(svd_gram(w, W, W, n, S));
        svd_chol_inv16(S, Rinv);
        RET(svd_mul(w, W, n, Rinv));
    }
    return 0;
}

static int svd_factors_ensure(Patch *P, int nb) {
    RET(P->svd_b.ensure(std::max<size_t>(1, (size_t)nb * P->d) * sizeof(double)));
    RET(P->svd_f.ensure(std::max<size_t>(1, (size_t)nb * P->T) * sizeof(double)));
    return P->svd_b0.ensure((size_t)P->d * sizeof(double));
}

// the fit of one patch: A over the BLOCK rows (CSC, K columns; K = 0: the reference's A = ones, C = zeros branch), traces through upload_centered
int bg_svd_fit_run(cnmfe_ctx *ctx, Patch *P, int nb, int32_t K, const int64_t *A_colptr, const int32_t *A_rowidx, const float *A_val, const float *C, int c_order) {
    const int64_t T = P->T, Tc = P->Tc, d_b = P->d_b, d = P->d;
    HostTrace ht(ctx, "bg_svd_fit");
    P->residual.invalidate();                                 // b, f, b0 change: whatever Ysig holds is no longer the residual under them
    P->svd_nb = -1;
    SvdStats &st = P->svd_stats; st = SvdStats(); st.nb = nb;
    DevBuf *S = ctx->svd;
    const bool has_a = K > 0 && A_colptr[K] > 0;
    if (has_a && A_colptr[K] >= (int64_t(1) << 31)) return fail(CNMFE_EUNSUPPORTED, "nnz(A) too large");
    int64_t ldc = 4;
    DevBuf &dC = ctx->tmp[0], &dCc = ctx->tmp[1], &dCm = ctx->tmp[2];
    const int *rowptr = nullptr, *rcol = nullptr; const float *rval = nullptr;
    if (has_a) {
        RET(upload_centered(ctx, dC, C, K, T, c_order, dCc, dCm, &ldc));
        HostCSR csr; csc_to_csr(d_b, K, A_colptr, A_rowidx, A_val, csr);
        RET(to_dev(ctx, S[SV_CP], A_colptr, (size_t)K + 1));
        RET(to_dev(ctx, S[SV_RI], A_rowidx, (size_t)A_colptr[K]));
        RET(to_dev(ctx, S[SV_CV], A_val, (size_t)A_colptr[K]));
        RET(to_dev(ctx, S[SV_RP], csr.rowptr));
        RET(to_dev(ctx, S[SV_RC], csr.col));
        RET(to_dev(ctx, S[SV_RV], csr.val));
        rowptr = S[SV_RP].as<int>(); rcol = S[SV_RC].as<int>(); rval = S[SV_RV].as<float>();
    }
    const int Ke = has_a ? K : 0;
    RET(svd_factors_ensure(P, nb));
    RET(S[SV_SMALL].ensure(512 * sizeof(double)));
    double *dSmall = S[SV_SMALL].as<double>();
    double *dRq = dSmall, *dSumG = dSmall + 16, *dFin = dSmall + 320;
    if (nb == 0) {                                              // fit_svd_model.m:20-25: b = f = 0, b0 = Ymean - A Cmean on the patch
        CK(hipMemsetAsync(dFin, 0, 48 * sizeof(double), ctx->st()));
        LAUNCH(ctx, "svd_b", k_svd_b, dim3((unsigned)((d + 255) / 256)), dim3(256), 0, (const double *)nullptr, 0, dFin, P->ymean_d.as<double>(), rowptr, rcol, rval,
               dCm.as<double>(), d, T, P->nr, P->nr_b, P->roff, P->coff, P->svd_b.as<double>(), P->svd_b0.as<double>());
        st.converged = 1; P->svd_nb = 0;
        return 0;
    }
    // the two passes' segments: enough workgroups to fill the device, partial sums added in segment order
    const int64_t gxP = (Tc + 15) / 16, Tpad = gxP * 64;
    int64_t nsegP = std::max<int64_t>(1, std::min<int64_t>((d_b + 127) / 128, (1024 + gxP - 1) / gxP));
    const int64_t pseg = (((d_b + nsegP - 1) / nsegP) + 127) & ~int64_t(127);
    nsegP = (d_b + pseg - 1) / pseg;
    const int64_t gxE = (d_b + 255) / 256;
    int64_t nsegE = std::max<int64_t>(1, std::min<int64_t>((Tc + 15) / 16, (1024 + gxE - 1) / gxE));
    const int64_t cseg = (((Tc + nsegE - 1) / nsegE) + 15) & ~int64_t(15);
    nsegE = (Tc + cseg - 1) / cseg;
    const int64_t nmax = std::max(d_b, T);
    const size_t part_n = std::max<size_t>({(size_t)(nsegP * Tpad * SVQ), (size_t)(nsegE * d_b * SVQ), (size_t)(((nmax + SVD_GRAM_ROWS - 1) / SVD_GRAM_ROWS) * 256)});
    RET(S[SV_PART].ensure(part_n * sizeof(double)));
    RET(S[SV_Q].ensure((size_t)d_b * SVQ * sizeof(double))); RET(S[SV_Z].ensure((size_t)d_b * SVQ * sizeof(double))); RET(S[SV_D].ensure((size_t)d_b * SVQ * sizeof(double)));
    RET(S[SV_G].ensure((size_t)T * SVQ * sizeof(double)));
    RET(S[SV_ATQ].ensure((size_t)std::max(1, Ke) * SVQ * sizeof(double))); RET(S[SV_CG].ensure((size_t)std::max(1, Ke) * SVQ * sizeof(double)));
    RET(S[SV_R].ensure((size_t)d_b * sizeof(double))); RET(S[SV_RS].ensure((size_t)(d_b + std::max(1, Ke)) * sizeof(double)));
    RET(S[SV_GRAM].ensure(256 * sizeof(double)));
    SvdWork w{ctx, P};
    double *dQ = S[SV_Q].as<double>(), *dZ = S[SV_Z].as<double>(), *dG = S[SV_G].as<double>(), *dD = S[SV_D].as<double>(), *dPart = S[SV_PART].as<double>();
    double *dR = S[SV_R].as<double>(), *dRs = S[SV_RS].as<double>(), *dCsum = dRs + d_b;
    const float4 *Yc4 = P->Yc4.as<float4>();
    // r = mean(Yc - A Cc, 2): analytically zero, in fp32 storage not (Yc is centred about the fp32 mean, Cc is rounded to fp32) -- one row-sum pass per fit
    LAUNCH(ctx, "svd_rowsum", k_svd_rowsum, dim3((unsigned)((d_b + 255) / 256)), dim3(256), 0, Yc4, d_b, Tc, dRs);
    if (Ke) LAUNCH(ctx, "svd_csum", k_svd_csum, dim3(Ke), dim3(256), 0, dCc.as<float>(), ldc, T, dCsum);
    LAUNCH(ctx, "svd_rmean", k_svd_rmean, dim3((unsigned)((d_b + 255) / 256)), dim3(256), 0, dRs, rowptr, rcol, rval, dCsum, d_b, T, dR);
    st.passes = 1;
    // the panel cannot be wider than the rank X can have (rows are centred: T - 1)
    const int qe = (int)std::min<int64_t>(SVQ, std::min<int64_t>(d_b, std::max<int64_t>(T - 1, 1)));
    LAUNCH(ctx, "svd_start", k_svd_start, dim3((unsigned)((d_b * SVQ + 255) / 256)), dim3(256), 0, dQ, d_b, qe);
    RET(svd_orth(w, dQ, d_b));
    const int max_iter = (int)std::max<int64_t>(1, ctx->opt("bg_svd_max_iter", 40));
    const double tol = std::pow(10.0, -(double)std::min<int64_t>(16, std::max<int64_t>(1, ctx->opt("bg_svd_tol_exp", 12))));
    double theta[SVQ] = {}, V[256], H[256], Sg[256];
    for (int it = 0; it < max_iter; ++it) {
        // G = X' Q
        if (Ke) LAUNCH(ctx, "svd_atq", k_svd_atq, dim3(Ke), dim3(256), 0, S[SV_CP].as<int64_t>(), S[SV_RI].as<int>(), S[SV_CV].as<float>(), dQ, S[SV_ATQ].as<double>());
        RET(svd_colsum(w, dQ, dR, d_b, dRq));
        LAUNCH(ctx, "svd_project", k_svd_project, dim3((unsigned)gxP, (unsigned)nsegP), dim3(256), 0, Yc4, d_b, Tc, dQ, pseg, dPart, Tpad);
        LAUNCH(ctx, "svd_g_finish", k_svd_g_finish, dim3((unsigned)((T * SVQ + 255) / 256)), dim3(256), 0, dPart, (int)nsegP, Tpad, T, dCc.as<float>(), ldc, Ke,
               S[SV_ATQ].as<double>(), dRq, dG);
        // the Ritz problem H = G'G = Q' M Q
        RET(svd_gram(w, dG, dG, T, H));
        svd_eigh16(H, theta, V);
        // Z = X G = M Q
        if (Ke) LAUNCH(ctx, "svd_cg", k_svd_cg, dim3(Ke), dim3(256), 0, dCc.as<float>(), ldc, T, dG, S[SV_CG].as<double>());
        RET(svd_colsum(w, dG, nullptr, T, dSumG));
        LAUNCH(ctx, "svd_expand", k_svd_expand, dim3((unsigned)gxE, (unsigned)nsegE), dim3(256), 0, Yc4, d_b, Tc, T, dG, cseg, dPart);
        LAUNCH(ctx, "svd_z_finish", k_svd_z_finish, dim3((unsigned)((d_b * SVQ + 255) / 256)), dim3(256), 0, dPart, (int)nsegE, d_b, rowptr, rcol, rval,
               S[SV_CG].as<double>(), dR, dSumG, dZ);
        st.passes += 2; st.iters = it + 1;
        // rotate the three panels onto the Ritz vectors: column i of Q -> u_i, of G -> s_i v_i, of Z -> M u_i
        RET(svd_mul(w, dQ, d_b, V)); RET(svd_mul(w, dZ, d_b, V)); RET(svd_mul(w, dG, T, V));
        // the residuals |M q_i - theta_i q_i|, measured
        RET(to_dev(ctx, S[SV_TH], theta, (size_t)SVQ));
        LAUNCH(ctx, "svd_axpy", k_svd_axpy, dim3((unsigned)((d_b * SVQ + 255) / 256)), dim3(256), 0, dZ, dQ, S[SV_TH].as<double>(), d_b, dD);
        RET(svd_gram(w, dD, dD, d_b, Sg));
        bool ok = true;
        const double th1 = std::fabs(theta[0]);
        for (int i = 0; i < nb; ++i) {
            const double r = std::sqrt(std::max(0.0, Sg[i * SVQ + i]));
            st.resid[i] = th1 > 0 ? r / th1 : 0.0;
            st.sv[i] = std::sqrt(std::fabs(theta[i]));
            if (!(r <= tol * th1)) ok = false;
        }
        if (ok) { st.converged = 1; break; }
        if (it + 1 == max_iter) break;                          // the cap: what the last iteration measured is what is handed out
        RET(svd_orth(w, dZ, d_b));
        std::swap(dQ, dZ);
    }
    ht.mark("iterations");
    // sign, then the factors on the patch
    double fin[48] = {};
    for (int i = 0; i < nb; ++i) fin[i] = std::sqrt(std::fabs(theta[i]));
    CK(hipMemcpyAsync(dFin, fin, 48 * sizeof(double), hipMemcpyHostToDevice, ctx->st()));
    CK(hipStreamSynchronize(ctx->st()));
    LAUNCH(ctx, "svd_sign", k_svd_sign, dim3(nb), dim3(256), 0, dQ, d_b, dFin + 16);
    RET(svd_colsum(w, dG, nullptr, T, dFin + 32));
    LAUNCH(ctx, "svd_f", k_svd_f, dim3((unsigned)((T * nb + 255) / 256)), dim3(256), 0, dG, T, nb, dFin, P->svd_f.as<double>());
    LAUNCH(ctx, "svd_b", k_svd_b, dim3((unsigned)((d + 255) / 256)), dim3(256), 0, dQ, nb, dFin, P->ymean_d.as<double>(), rowptr, rcol, rval, dCm.as<double>(), d, T,
           P->nr, P->nr_b, P->roff, P->coff, P->svd_b.as<double>(), P->svd_b0.as<double>());
    P->svd_nb = nb;
    return 0;
}

// transplant a saved background: b d x nb (column-major), f nb x T (row-major), b0 d
int bg_svd_set_run(cnmfe_ctx *ctx, Patch *P, int nb, const double *b, const double *f, const double *b0) {
    P->residual.invalidate();
    P->svd_nb = -1; P->svd_stats = SvdStats(); P->svd_stats.nb = nb;
    RET(svd_factors_ensure(P, nb));
    if (nb > 0) {
        CK(hipMemcpyAsync(P->svd_b.p, b, (size_t)nb * P->d * sizeof(double), hipMemcpyHostToDevice, ctx->st()));
        CK(hipMemcpyAsync(P->svd_f.p, f, (size_t)nb * P->T * sizeof(double), hipMemcpyHostToDevice, ctx->st()));
    }
    CK(hipMemcpyAsync(P->svd_b0.p, b0, (size_t)P->d * sizeof(double), hipMemcpyHostToDevice, ctx->st()));
    CK(hipStreamSynchronize(ctx->st()));
    P->svd_nb = nb;
    return 0;
}

int bg_svd_get_run(cnmfe_ctx *ctx, Patch *P, double *b, double *f, double *b0) {
    const int nb = P->svd_nb;
    if (nb > 0 && b) CK(hipMemcpyAsync(b, P->svd_b.p, (size_t)nb * P->d * sizeof(double), hipMemcpyDeviceToHost, ctx->st()));
    if (nb > 0 && f) CK(hipMemcpyAsync(f, P->svd_f.p, (size_t)nb * P->T * sizeof(double), hipMemcpyDeviceToHost, ctx->st()));
    if (b0) CK(hipMemcpyAsync(b0, P->svd_b0.p, (size_t)P->d * sizeof(double), hipMemcpyDeviceToHost, ctx->st()));
    CK(hipStreamSynchronize(ctx->st()));
    return 0;
}

// Ysig of the patch under the kept b, f, b0: resident, source SRC_LOWRANK, no applied and no pending term -- the updates run on it through their non-virtual branch
int bg_svd_resid_run(cnmfe_ctx *ctx, Patch *P, float *Ysig_out, int out_memspace) {
    ResidualState &rs = P->residual;
    ++rs.gen;
    const rplan::LowrankPlan plan = rplan::lowrank_plan({rs.form, rs.source, P->ysig.p != nullptr});
    if (plan.sweep) {
        rs.invalidate();
        RET(P->ysig.ensure((size_t)P->d * P->Tc * sizeof(float4)));
        LAUNCH(ctx, "lowrank_resid", k_lowrank_resid, dim3((unsigned)((P->d + 255) / 256), (unsigned)P->Tc), dim3(256), 0, P->Yc4.as<float4>(), P->ymean_f.as<float>(),
               P->svd_b0.as<double>(), P->svd_b.as<double>(), P->svd_f.as<double>(), P->svd_nb, P->d, P->d_b, P->T, P->nr, P->nr_b, P->roff, P->coff, P->ysig.as<float4>());
        rs.applied.set(false, 4, 0); rs.has_pending = false;
        rs.source = rplan::SRC_LOWRANK; rs.form = rplan::RESIDENT;
    }
    if (Ysig_out) RET(ysig_export(ctx, P, P->ysig, Ysig_out, out_memspace));
    return 0;
}

}  // namespace cnmfe
