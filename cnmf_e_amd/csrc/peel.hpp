// (g) greedy initialisation: the SEQUENTIAL half of greedyROI_endoscope as a per-patch session
//   endoscope/greedyROI_endoscope.m:119-145 (open), :287-311 + endoscope/extract_ac.m:19-58 (extract), :378-402 (apply)
// Included by deconv.hip below seed.hpp: open runs the seed pipeline once (k_seed_filter / k_seed_stats / k_seed_corr / k_seed_cn) and keeps
//   HY   the filtered block, trend and median subtracted IN PLACE by the arithmetic k_seed_stats / k_seed_corr use (seed_detrend, then the float subtraction)
//   Sn   GetSn of every pixel's HY trace, fixed for the session (:132)
//   Yw   a working copy of the centred block video (nk > 1: Yc - (Yc Q) Q'), which the peel subtracts from
// The peel is sequential over neurons; one step is data-parallel over a (2 gSiz + 1)^2 or (4 gSiz + 1)^2 pixel box times all frames.  A pixel's trace is strided
// by d_b float4s and a box column is the contiguous run, so the box kernels put 64 lanes on the box rows and one wave on each of 4 interleaved frame quads:
// workgroup = (box column, frame chunk).  Every sum is a per-lane fp64 partial, and the partials are added in ascending (chunk, wave) order by a second small
// kernel: two identical sessions are bit-identical.  Only frames t < n enter anything (the last quad's padding does not).
// Frames: 64 <= n <= WELCH_TMAX = 147456.  Every kernel but two takes n as a loop bound (64-bit offsets q * d_b; grid.y = frame chunks <= 32, grid.x = ceil(n / 4)
// <= 36864 for k_peel_traces).  The two that hold a whole trace -- k_seed_stats (seed.hpp) and k_peel_trace_stats -- have a long flavour beyond 20416 frames whose
// trace stays in global memory (welch_cfg, deconv.hip); k_peel_trace_stats_long needs no scratch: ci already lies there as doubles.
// A session runs on the geometry of its source video (PeelSession::d / nr / nc): the block for cnmfe_peel_open, the PATCH and its residual video
// Yres = Ysig - A C (k_peel_yres) for cnmfe_peel_open_residual, the second pass of @Sources2D/initComponents_residual_parallel.m:186-220; under
// background_model = 'svd' the same geometry and Yres = Y - A C - (b f + b0) straight from the centred video (k_peel_yres_lowrank) for cnmfe_peel_open_lowrank.
#pragma once

namespace cnmfe {

constexpr int PEEL_GMAX = 20;                         // gSiz limit: the extract box is at most 41 x 41 pixels, the apply box 81 x 81
constexpr int PEEL_QL = 4;                            // frame-quad lanes of a box kernel (one wave each); 64 row lanes
constexpr int PEEL_NCH = 32;                          // at most this many frame chunks

struct PeelBox { int r0, c0, nr, nc; };               // 0-based origin inside the block, size

__device__ __forceinline__ int64_t peel_pix(const PeelBox &b, int i, int nr_b) { return (int64_t)(b.c0 + i / b.nr) * nr_b + b.r0 + i % b.nr; }

// (k_peel_hy_final, which turns the filtered block into HY of greedyROI_endoscope.m:130 in place, sits in seed.hpp beside the two kernels whose arithmetic it repeats)

// Yw = Yc - (Yc Q) Q' (initComponents_parallel.m:341-343 -> detrend_data.m:26-29 on the raw video: the pixel mean lies in the span of the splines), one
// workgroup per block pixel; the padding frames become 0
__global__ void __launch_bounds__(256) k_peel_yw_detrend(const float4 *__restrict__ yc4, float4 *__restrict__ yw4, int64_t d_b, int n,
                                                         const double *__restrict__ Q, int M) {
    __shared__ double red[4];
    __shared__ double coef[SEED_MMAX];
    const int64_t p = blockIdx.x;
    const int tid = threadIdx.x, nq = (n + 3) / 4;
    for (int m = 0; m < M; ++m) {
        double s = 0;
        for (int q = tid; q < nq; q += 256) {
            const float4 v4 = yc4[(int64_t)q * d_b + p];
            const float v[4] = {v4.x, v4.y, v4.z, v4.w};
            for (int j = 0; j < 4; ++j) { const int t = 4 * q + j; if (t < n) s = fma(Q[(int64_t)m * n + t], (double)v[j], s); }
        }
        s = block_sum(s, red);
        if (tid == 0) coef[m] = s;
    }
    __syncthreads();
    for (int q = tid; q < nq; q += 256) {
        const float4 v4 = yc4[(int64_t)q * d_b + p];
        float v[4] = {v4.x, v4.y, v4.z, v4.w};
        for (int j = 0; j < 4; ++j) { const int t = 4 * q + j; v[j] = t < n ? seed_detrend(v[j], coef, Q + t, n, M) : 0.f; }
        yw4[(int64_t)q * d_b + p] = make_float4(v[0], v[1], v[2], v[3]);
    }
}

// The source video of a residual session (@Sources2D/initComponents_residual_parallel.m:199,206): Yres = Ysig - A(patch, ind) C(ind, :) off the resident residual,
// which is only read.  One thread per patch pixel and frame quad: the pixel's stored neurons (CSR row, ascending column) are summed in fp64 and the difference
// is rounded once; the padding frames of the last quad become 0.  The result IS the session's working copy Yw: until the first apply Yw equals Yres bit for
// bit, so the seed pipeline and the export of the open read it there and no third video is kept.  16 bytes read, 16 written per (pixel, quad), coalesced
// over pixels; the trace quads C(k, 4q..) of a wave's few neurons come from L2.  rowptr == nullptr: no footprint in the patch, a copy.
__global__ void __launch_bounds__(256) k_peel_yres(const float4 *__restrict__ ysig4, int64_t d, int n, int qchunk, const int *__restrict__ rowptr,
                                                   const int *__restrict__ col, const float *__restrict__ val, const float *__restrict__ C, int64_t ldc,
                                                   float4 *__restrict__ yw4) {
    const int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (p >= d) return;
    const int nq = (n + 3) / 4, q0 = (int)blockIdx.y * qchunk, q1 = min(nq, q0 + qchunk);
    const int e0 = rowptr ? rowptr[p] : 0, e1 = rowptr ? rowptr[p + 1] : 0;
    for (int q = q0; q < q1; ++q) {
        const float4 y4 = ysig4[(int64_t)q * d + p];
        double s[4] = {0.0, 0.0, 0.0, 0.0};
        for (int e = e0; e < e1; ++e) {
            const double a = (double)val[e];
            const float4 c4 = *reinterpret_cast<const float4 *>(C + (int64_t)col[e] * ldc + 4 * (int64_t)q);
            s[0] = fma(a, (double)c4.x, s[0]); s[1] = fma(a, (double)c4.y, s[1]); s[2] = fma(a, (double)c4.z, s[2]); s[3] = fma(a, (double)c4.w, s[3]);
        }
        float v[4] = {(float)((double)y4.x - s[0]), (float)((double)y4.y - s[1]), (float)((double)y4.z - s[2]), (float)((double)y4.w - s[3])};
#pragma unroll
        for (int j = 0; j < 4; ++j) if (4 * q + j >= n) v[j] = 0.f;
        yw4[(int64_t)q * d + p] = make_float4(v[0], v[1], v[2], v[3]);
    }
}

// The same video under background_model = 'svd' (@Sources2D/initComponents_residual_parallel.m:107-122,195-199,224-227): Yres = Y(patch) - A(patch, ind) C(ind, :)
// - (b f + b0), written straight from the centred BLOCK video -- no Ysig is realised.  Per (patch pixel, frame quad)
//     Yc + (ymean_f - b0) - [sum_i b(m, i) f(i, t) + sum_e a_e C(col_e, t)]
// in fp64: one fma chain, i ascending, then the pixel's CSR row ascending, ONE rounding to fp32; the padding frames of the last quad become 0.  16 bytes read
// (block-indexed through roff / coff / nr_b, as k_lowrank_resid reads them), 16 written; the pixel's row of b (at most PEEL_LR_NB doubles) stays in registers over
// the quads of its chunk; f(i, 4q ..) is the same address for every lane of the workgroup and comes from L2 like the trace quads.  f's rows are T doubles apart, so
// they are read as scalars with k_lowrank_resid's guards on the last quad.  rowptr == nullptr: no footprint in the patch; nb = 0: no b f.
constexpr int PEEL_LR_NB = 8;                         // = SVD_NB_MAX (bg_svd.hpp lives in another translation unit)
__global__ void __launch_bounds__(256) k_peel_yres_lowrank(const float4 *__restrict__ yc4, const float *__restrict__ ymean_f, const double *__restrict__ b0,
                                                           const double *__restrict__ b, const double *__restrict__ f, int nb, int64_t d, int64_t d_b, int n, int nr,
                                                           int nr_b, int roff, int coff, int qchunk, const int *__restrict__ rowptr, const int *__restrict__ col,
                                                           const float *__restrict__ val, const float *__restrict__ C, int64_t ldc, float4 *__restrict__ yw4) {
    const int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (p >= d) return;
    const int64_t pb = (int64_t)((int)(p / nr) + coff) * nr_b + (int)(p % nr) + roff;
    const int nq = (n + 3) / 4, q0 = (int)blockIdx.y * qchunk, q1 = min(nq, q0 + qchunk);
    const int e0 = rowptr ? rowptr[p] : 0, e1 = rowptr ? rowptr[p + 1] : 0;
    const double dl = (double)ymean_f[pb] - b0[p];
    double bm[PEEL_LR_NB];
#pragma unroll
    for (int i = 0; i < PEEL_LR_NB; ++i) bm[i] = i < nb ? b[(int64_t)i * d + p] : 0.0;
    for (int q = q0; q < q1; ++q) {
        const float4 y4 = yc4[(int64_t)q * d_b + pb];
        const int t = 4 * q;
        double s[4] = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
        for (int i = 0; i < PEEL_LR_NB; ++i)
            if (i < nb) {
                const double *fr = f + (int64_t)i * n + t;
                s[0] = fma(bm[i], fr[0], s[0]);
                if (t + 1 < n) s[1] = fma(bm[i], fr[1], s[1]);
                if (t + 2 < n) s[2] = fma(bm[i], fr[2], s[2]);
                if (t + 3 < n) s[3] = fma(bm[i], fr[3], s[3]);
            }
        for (int e = e0; e < e1; ++e) {
            const double a = (double)val[e];
            const float4 c4 = *reinterpret_cast<const float4 *>(C + (int64_t)col[e] * ldc + 4 * (int64_t)q);
            s[0] = fma(a, (double)c4.x, s[0]); s[1] = fma(a, (double)c4.y, s[1]); s[2] = fma(a, (double)c4.z, s[2]); s[3] = fma(a, (double)c4.w, s[3]);
        }
        float v[4] = {(float)(((double)y4.x + dl) - s[0]), (float)(((double)y4.y + dl) - s[1]), (float)(((double)y4.z + dl) - s[2]), (float)(((double)y4.w + dl) - s[3])};
#pragma unroll
        for (int j = 0; j < 4; ++j) if (t + j >= n) v[j] = 0.f;
        yw4[(int64_t)q * d + p] = make_float4(v[0], v[1], v[2], v[3]);
    }
}

// ---- extract ---------------------------------------------------------------------------------------------------------------------------------------------
// corr(y0', HY_box') (extract_ac.m:22), the moments: per (box pixel, chunk, wave) sum x, sum x^2, sum x y0.  part[((chunk * 4 + wave) * npix + i) * 3 + .]
__global__ void __launch_bounds__(256) k_peel_corr_part(const float4 *__restrict__ hy4, int64_t d_b, int nr_b, PeelBox b, int64_t pctr, int n, int qchunk,
                                                        double *__restrict__ part) {
    const int tid = threadIdx.x, tr = tid & 63, tq = tid >> 6, col = (int)blockIdx.x;
    const int nq = (n + 3) / 4, q0 = (int)blockIdx.y * qchunk, q1 = min(nq, q0 + qchunk), npix = b.nr * b.nc;
    for (int row = tr; row < b.nr; row += 64) {
        const int64_t p = (int64_t)(b.c0 + col) * nr_b + b.r0 + row;
        double sx = 0, sxx = 0, sxy = 0;
        for (int q = q0 + tq; q < q1; q += PEEL_QL) {
            const float4 x4 = hy4[(int64_t)q * d_b + p], y4 = hy4[(int64_t)q * d_b + pctr];
            const float x[4] = {x4.x, x4.y, x4.z, x4.w}, y[4] = {y4.x, y4.y, y4.z, y4.w};
#pragma unroll
            for (int j = 0; j < 4; ++j)
                if (4 * q + j < n) { const double xv = (double)x[j]; sx += xv; sxx = fma(xv, xv, sxx); sxy = fma(xv, (double)y[j], sxy); }
        }
        double *o = part + ((int64_t)((int)blockIdx.y * PEEL_QL + tq) * npix + col * b.nr + row) * 3;
        o[0] = sx; o[1] = sxx; o[2] = sxy;
    }
}

// One workgroup: Pearson's r of every box pixel with the centre (a constant trace: 0 / 0 = NaN, as corr gives), then the two pixel sets in ascending box
// order: {corr > 0.9} (extract_ac.m:23) and {corr < 0.3} (:37).  cnt[0], cnt[1] = their sizes.
__global__ void __launch_bounds__(256) k_peel_corr_fin(const double *__restrict__ part, int npart, int npix, int ictr, int n, double *__restrict__ corr,
                                                       int *__restrict__ hi, int *__restrict__ lo, int *__restrict__ cnt) {
    const int tid = threadIdx.x;
    double sy = 0, syy = 0;
    for (int k = 0; k < npart; ++k) { const double *o = part + ((int64_t)k * npix + ictr) * 3; sy += o[0]; syy += o[1]; }
    const double vy = syy - sy * sy / (double)n;
    for (int i = tid; i < npix; i += 256) {
        double sx = 0, sxx = 0, sxy = 0;
        for (int k = 0; k < npart; ++k) { const double *o = part + ((int64_t)k * npix + i) * 3; sx += o[0]; sxx += o[1]; sxy += o[2]; }
        const double vx = sxx - sx * sx / (double)n;
        corr[i] = (sxy - sx * sy / (double)n) / sqrt(vx * vy);
    }
    __threadfence_block();
    __syncthreads();
    if (tid == 0) {
        int nh = 0, nl = 0;
        for (int i = 0; i < npix; ++i) { const double r = corr[i]; if (r > 0.9) hi[nh++] = i; if (r < 0.3) lo[nl++] = i; }
        cnt[0] = nh; cnt[1] = nl;
    }
}

// the two adjacent order statistics k, k + 1 of N doubles in LDS: select_pair on 64-bit keys (eight 256-bin passes)
__device__ __forceinline__ unsigned long long dkey(double x) { const unsigned long long u = (unsigned long long)__double_as_longlong(x); return (u >> 63) ? ~u : (u | (1ull << 63)); }
__device__ __forceinline__ double dkey_inv(unsigned long long k) { return __longlong_as_double((long long)((k >> 63) ? (k & ~(1ull << 63)) : ~k)); }
__device__ void select_pair64(const double *y, int N, int k, int *hist /* 264 ints of LDS, 8-byte aligned */, double &vk, double &vk1) {
    const int tid = threadIdx.x, NTH = (int)blockDim.x;
    unsigned long long prefix = 0, known = 0;
    int kk = k, cnt_eq = 0;
    for (int shift = 56; shift >= 0; shift -= 8) {
        if (tid < 256) hist[tid] = 0;
        __syncthreads();
        for (int t = tid; t < N; t += NTH) { const unsigned long long key = dkey(y[t]); if ((key & known) == prefix) atomicAdd(&hist[(int)((key >> shift) & 255)], 1); }
        __syncthreads();
        if (tid == 0) {
            int acc = 0, b = 0;
            for (; b < 255; ++b) { const int h = hist[b]; if (acc + h > kk) break; acc += h; }
            hist[256] = b; hist[257] = kk - acc; hist[258] = hist[b];
        }
        __syncthreads();
        prefix |= (unsigned long long)hist[256] << shift; known |= 255ull << shift; kk = hist[257]; cnt_eq = hist[258];
        __syncthreads();
    }
    vk = dkey_inv(prefix);
    if (kk + 1 < cnt_eq) { vk1 = vk; return; }
    unsigned long long mn = ~0ull;
    for (int t = tid; t < N; t += NTH) { const unsigned long long key = dkey(y[t]); if (key > prefix && key < mn) mn = key; }
    for (int o = 32; o > 0; o >>= 1) { const unsigned long long other = __shfl_xor(mn, o); mn = other < mn ? other : mn; }
    unsigned long long *wmin = reinterpret_cast<unsigned long long *>(hist);
    if ((tid & 63) == 0) wmin[tid >> 6] = mn;
    __syncthreads();
    unsigned long long r = wmin[0];
    for (int w = 1; w < (NTH >> 6); ++w) r = wmin[w] < r ? wmin[w] : r;
    __syncthreads();
    vk1 = r == ~0ull ? vk : dkey_inv(r);
}

// One workgroup per frame quad: ci(t) = mean(HY(corr > 0.9, t)) (extract_ac.m:27) and y_bg(t) = median(Y(corr < 0.3, t)) (:37) with Y = Yw + Ybar in fp64
// (ymean == nullptr: the detrended video, no mean).  An empty set gives NaN for either.
__global__ void __launch_bounds__(256) k_peel_traces(const float4 *__restrict__ hy4, const float4 *__restrict__ yw4, const double *__restrict__ ymean,
                                                     int64_t d_b, int nr_b, PeelBox b, const int *__restrict__ hi, const int *__restrict__ lo,
                                                     const int *__restrict__ cnt, int n, double *__restrict__ ci, double *__restrict__ ybg) {
    extern __shared__ __attribute__((aligned(16))) double peel_sm[];
    __shared__ double red[4];
    const int tid = threadIdx.x, q = (int)blockIdx.x, npix = b.nr * b.nc, nhi = cnt[0], nlo = cnt[1];
    double *vals = peel_sm;
    int *hist = reinterpret_cast<int *>(peel_sm + (size_t)4 * npix);
    double s[4] = {0.0, 0.0, 0.0, 0.0};
    for (int i = tid; i < nhi; i += 256) {
        const float4 v = hy4[(int64_t)q * d_b + peel_pix(b, hi[i], nr_b)];
        s[0] += (double)v.x; s[1] += (double)v.y; s[2] += (double)v.z; s[3] += (double)v.w;
    }
    for (int j = 0; j < 4; ++j) {
        const double sj = block_sum(s[j], red);
        if (tid == 0 && 4 * q + j < n) ci[4 * q + j] = sj / (double)nhi;
    }
    for (int i = tid; i < nlo; i += 256) {
        const int64_t p = peel_pix(b, lo[i], nr_b);
        const float4 v = yw4[(int64_t)q * d_b + p];
        const double m = ymean ? ymean[p] : 0.0;
        vals[i] = (double)v.x + m; vals[npix + i] = (double)v.y + m; vals[2 * npix + i] = (double)v.z + m; vals[3 * npix + i] = (double)v.w + m;
    }
    __syncthreads();
    for (int j = 0; j < 4; ++j) {
        const int t = 4 * q + j;
        if (t >= n) break;
        if (nlo == 0) { if (tid == 0) ybg[t] = __longlong_as_double(0x7ff8000000000000ll); continue; }
        double vk, vk1;
        select_pair64(vals + (size_t)j * npix, nlo, (nlo - 1) / 2, hist, vk, vk1);
        if (tid == 0) ybg[t] = (nlo & 1) ? vk : 0.5 * (vk + vk1);
    }
}

__device__ __forceinline__ double peel_block_max(double v, double *red) {
    const int tid = threadIdx.x;
    for (int o = 32; o > 0; o >>= 1) v = fmax(v, __shfl_xor(v, o));
    __syncthreads();
    if ((tid & 63) == 0) red[tid >> 6] = v;
    __syncthreads();
    const double r = fmax(fmax(red[0], red[1]), fmax(red[2], red[3]));
    __syncthreads();
    return r;
}

// One workgroup: the means and centred second moments of (y_bg, ci) for the regression, and the numbers the host's tests read --
//   st[0] max(diff(y0)), st[1] std(diff(y0)) (greedyROI_endoscope.m:287-293), st[2] norm(ci) (extract_ac.m:29), st[3] GetSn(ci) (:89), st[4], st[5] the set sizes
// mom = mean y_bg, mean ci, S_bb, S_bc, S_cc.  LDS: the layout of k_seed_stats (the trace as floats | the Welch transform).
__global__ void __launch_bounds__(256) k_peel_trace_stats(DeconvCfg c, const float4 *__restrict__ hy4, int64_t d_b, int64_t pctr, const double *__restrict__ ci,
                                                          const double *__restrict__ ybg, const int *__restrict__ cnt, double *__restrict__ mom,
                                                          double *__restrict__ st) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    __shared__ double red[4];
    const int tid = threadIdx.x, n = c.T;
    const int Tal = (n + 3) & ~3;
    float *y = lds, *scr = lds + Tal;
    double sb = 0, sc = 0, s2 = 0;
    for (int t = tid; t < n; t += 256) { const double cv = ci[t]; sb += ybg[t]; sc += cv; s2 = fma(cv, cv, s2); y[t] = (float)cv; }
    const double mb = block_sum(sb, red) / (double)n, mc = block_sum(sc, red) / (double)n, nrm = sqrt(block_sum(s2, red));
    double sbb = 0, sbc = 0, scc = 0;
    for (int t = tid; t < n; t += 256) { const double bv = ybg[t] - mb, cv = ci[t] - mc; sbb = fma(bv, bv, sbb); sbc = fma(bv, cv, sbc); scc = fma(cv, cv, scc); }
    sbb = block_sum(sbb, red); sbc = block_sum(sbc, red); scc = block_sum(scc, red);
    // diff(y0): n - 1 differences, std with N - 1 = n - 2 in the denominator
    auto y0 = [&](int t) { return (double)reinterpret_cast<const float *>(hy4 + (int64_t)(t >> 2) * d_b + pctr)[t & 3]; };
    double dmx = -INFINITY, ds = 0;
    for (int t = tid; t < n - 1; t += 256) { const double dv = y0(t + 1) - y0(t); dmx = fmax(dmx, dv); ds += dv; }
    dmx = peel_block_max(dmx, red);
    const double dmean = block_sum(ds, red) / (double)(n - 1);
    double dv2 = 0;
    for (int t = tid; t < n - 1; t += 256) { const double dv = (y0(t + 1) - y0(t)) - dmean; dv2 = fma(dv, dv, dv2); }
    const double dstd = sqrt(block_sum(dv2, red) / (double)(n - 2));
    const double sn = get_sn(y, c, scr, red, false);         // (block_sum's barriers have published y)
    if (tid == 0) {
        mom[0] = mb; mom[1] = mc; mom[2] = sbb; mom[3] = sbc; mom[4] = scc;
        st[0] = dmx; st[1] = dstd; st[2] = nrm; st[3] = sn; st[4] = (double)cnt[0]; st[5] = (double)cnt[1];
    }
}

// The long flavour (welch_cfg, deconv.hip): ci stays where it is, in global memory as doubles, and get_sn reads it through an accessor that rounds each sample to
// float on the fly -- the values the LDS copy holds; LDS is the transform alone.  Every sum as in k_peel_trace_stats: equal bits where both run.
struct PeelCiAcc {
    const double *ci;
    __device__ __forceinline__ float operator[](int t) const { return (float)ci[t]; }
};
template <bool SPLIT>
__global__ void __launch_bounds__(256) k_peel_trace_stats_long(DeconvCfg c, float *__restrict__ tabs, const float4 *__restrict__ hy4, int64_t d_b, int64_t pctr,
                                                               const double *__restrict__ ci, const double *__restrict__ ybg, const int *__restrict__ cnt,
                                                               double *__restrict__ mom, double *__restrict__ st) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    __shared__ double red[4];
    const int tid = threadIdx.x, n = c.T;
    double sb = 0, sc = 0, s2 = 0;
    for (int t = tid; t < n; t += 256) { const double cv = ci[t]; sb += ybg[t]; sc += cv; s2 = fma(cv, cv, s2); }
    const double mb = block_sum(sb, red) / (double)n, mc = block_sum(sc, red) / (double)n, nrm = sqrt(block_sum(s2, red));
    double sbb = 0, sbc = 0, scc = 0;
    for (int t = tid; t < n; t += 256) { const double bv = ybg[t] - mb, cv = ci[t] - mc; sbb = fma(bv, bv, sbb); sbc = fma(bv, cv, sbc); scc = fma(cv, cv, scc); }
    sbb = block_sum(sbb, red); sbc = block_sum(sbc, red); scc = block_sum(scc, red);
    auto y0 = [&](int t) { return (double)reinterpret_cast<const float *>(hy4 + (int64_t)(t >> 2) * d_b + pctr)[t & 3]; };
    double dmx = -INFINITY, ds = 0;
    for (int t = tid; t < n - 1; t += 256) { const double dv = y0(t + 1) - y0(t); dmx = fmax(dmx, dv); ds += dv; }
    dmx = peel_block_max(dmx, red);
    const double dmean = block_sum(ds, red) / (double)(n - 1);
    double dv2 = 0;
    for (int t = tid; t < n - 1; t += 256) { const double dv = (y0(t + 1) - y0(t)) - dmean; dv2 = fma(dv, dv, dv2); }
    const double dstd = sqrt(block_sum(dv2, red) / (double)(n - 2));
    const double sn = get_sn_long<SPLIT>(PeelCiAcc{ci}, c, lds, red, tabs);
    if (tid == 0) {
        mom[0] = mb; mom[1] = mc; mom[2] = sbb; mom[3] = sbc; mom[4] = scc;
        st[0] = dmx; st[1] = dstd; st[2] = nrm; st[3] = sn; st[4] = (double)cnt[0]; st[5] = (double)cnt[1];
    }
}

// X = [1, y_bg', ci'], temp = (X'X) \ (X'Y') (extract_ac.m:55-57): per box pixel the two centred cross moments sum (y_bg - mean) Y, sum (ci - mean) Y
// part[((chunk * 4 + wave) * npix + i) * 2 + .]
__global__ void __launch_bounds__(256) k_peel_mom_part(const float4 *__restrict__ yw4, int64_t d_b, int nr_b, PeelBox b, const double *__restrict__ ci,
                                                       const double *__restrict__ ybg, const double *__restrict__ mom, int n, int qchunk,
                                                       double *__restrict__ part) {
    const int tid = threadIdx.x, tr = tid & 63, tq = tid >> 6, col = (int)blockIdx.x;
    const int nq = (n + 3) / 4, q0 = (int)blockIdx.y * qchunk, q1 = min(nq, q0 + qchunk), npix = b.nr * b.nc;
    const double mb = mom[0], mc = mom[1];
    for (int row = tr; row < b.nr; row += 64) {
        const int64_t p = (int64_t)(b.c0 + col) * nr_b + b.r0 + row;
        double sby = 0, scy = 0;
        for (int q = q0 + tq; q < q1; q += PEEL_QL) {
            const float4 x4 = yw4[(int64_t)q * d_b + p];
            const float x[4] = {x4.x, x4.y, x4.z, x4.w};
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int t = 4 * q + j;
                if (t < n) { const double xv = (double)x[j]; sby = fma(ybg[t] - mb, xv, sby); scy = fma(ci[t] - mc, xv, scy); }
            }
        }
        double *o = part + ((int64_t)((int)blockIdx.y * PEEL_QL + tq) * npix + col * b.nr + row) * 2;
        o[0] = sby; o[1] = scy;
    }
}

// ai = max(0, temp(3, :)') (extract_ac.m:58) from the 2 x 2 system of the centred regressors -- the same row as the raw 3 x 3 solve, whose intercept
// column (the baseline is ~1000) it eliminates exactly.  max(0, NaN) = 0 as in MATLAB.
__global__ void __launch_bounds__(256) k_peel_ai_fin(const double *__restrict__ part, int npart, int npix, const double *__restrict__ mom, double *__restrict__ ai) {
    const int i = (int)blockIdx.x * 256 + threadIdx.x;
    if (i >= npix) return;
    double sby = 0, scy = 0;
    for (int k = 0; k < npart; ++k) { const double *o = part + ((int64_t)k * npix + i) * 2; sby += o[0]; scy += o[1]; }
    const double sbb = mom[2], sbc = mom[3], scc = mom[4];
    const double beta = (sbb * scy - sbc * sby) / (sbb * scc - sbc * sbc);
    ai[i] = beta > 0.0 ? beta : 0.0;
}

// ---- apply -----------------------------------------------------------------------------------------------------------------------------------------------
// V(box, :) -= a ci (greedyROI_endoscope.m:378 on Yw, :385-387 on HY): the product and the difference in fp64, rounded once
__global__ void __launch_bounds__(256) k_peel_rank1(float4 *__restrict__ v4, int64_t d_b, int nr_b, PeelBox b, const double *__restrict__ a,
                                                    const double *__restrict__ ci, int n, int qchunk) {
    const int tid = threadIdx.x, tr = tid & 63, tq = tid >> 6, col = (int)blockIdx.x;
    const int nq = (n + 3) / 4, q0 = (int)blockIdx.y * qchunk, q1 = min(nq, q0 + qchunk);
    for (int row = tr; row < b.nr; row += 64) {
        const double av = a[col * b.nr + row];
        if (av == 0.0) continue;
        const int64_t p = (int64_t)(b.c0 + col) * nr_b + b.r0 + row;
        for (int q = q0 + tq; q < q1; q += PEEL_QL) {
            const float4 x4 = v4[(int64_t)q * d_b + p];
            float x[4] = {x4.x, x4.y, x4.z, x4.w};
#pragma unroll
            for (int j = 0; j < 4; ++j) { const int t = 4 * q + j; if (t < n) x[j] = (float)fma(-av, ci[t], (double)x[j]); }
            v4[(int64_t)q * d_b + p] = make_float4(x[0], x[1], x[2], x[3]);
        }
    }
}

// per pixel of the updated box: max(HY_box, [], 2) (:391) and the sums of HY_box_thr (:396-397; HY < sig Sn compared in fp64, as k_seed_stats does)
// part[((chunk * 4 + wave) * npix + i) * 3 + .] = max, sum, sum of squares
__global__ void __launch_bounds__(256) k_peel_box_part(const float4 *__restrict__ hy4, int64_t d_b, int nr_b, PeelBox b, const double *__restrict__ sn, double sig,
                                                       int n, int qchunk, double *__restrict__ part) {
    const int tid = threadIdx.x, tr = tid & 63, tq = tid >> 6, col = (int)blockIdx.x;
    const int nq = (n + 3) / 4, q0 = (int)blockIdx.y * qchunk, q1 = min(nq, q0 + qchunk), npix = b.nr * b.nc;
    for (int row = tr; row < b.nr; row += 64) {
        const int64_t p = (int64_t)(b.c0 + col) * nr_b + b.r0 + row;
        const double thr = sig * sn[p];
        double mx = -INFINITY, s1 = 0, s2 = 0;
        for (int q = q0 + tq; q < q1; q += PEEL_QL) {
            const float4 x4 = hy4[(int64_t)q * d_b + p];
            const float x[4] = {x4.x, x4.y, x4.z, x4.w};
#pragma unroll
            for (int j = 0; j < 4; ++j)
                if (4 * q + j < n) { const double v = (double)x[j]; mx = fmax(mx, v); const double w = v < thr ? 0.0 : v; s1 += w; s2 = fma(w, w, s2); }
        }
        double *o = part + ((int64_t)((int)blockIdx.y * PEEL_QL + tq) * npix + col * b.nr + row) * 3;
        o[0] = mx; o[1] = s1; o[2] = s2;
    }
}

// tmp_PNR (:392-393) and the record k_peel_corr8 standardises with: threshold, mean, 1 / rms (correlation_image.m:32,47-48; rms 0 -> 1)
__global__ void __launch_bounds__(256) k_peel_box_rec(const double *__restrict__ part, int npart, PeelBox b, int nr_b, const double *__restrict__ sn, double sig,
                                                      double min_pnr, int n, double *__restrict__ rec, float *__restrict__ pnr) {
    const int i = (int)blockIdx.x * 256 + threadIdx.x, npix = b.nr * b.nc;
    if (i >= npix) return;
    double mx = -INFINITY, s1 = 0, s2 = 0;
    for (int k = 0; k < npart; ++k) { const double *o = part + ((int64_t)k * npix + i) * 3; mx = fmax(mx, o[0]); s1 += o[1]; s2 += o[2]; }
    const double s = sn[peel_pix(b, i, nr_b)];
    const double mean = s1 / (double)n, var = fmax(s2 / (double)n - mean * mean, 0.0), rms = sqrt(var);
    rec[3 * i] = sig * s; rec[3 * i + 1] = mean; rec[3 * i + 2] = rms == 0.0 ? 1.0 : 1.0 / rms;
    const double r = mx / s;
    pnr[i] = (r != r || r < min_pnr) ? 0.f : (float)r;
}

// k_seed_corr on the box taken as a whole image (:400, correlation_image(HY_box_thr, [1, 2], nr2, nc2)): neighbours outside the BOX are the zero padding
__global__ void __launch_bounds__(256) k_peel_corr8(const float4 *__restrict__ hy4, int64_t d_b, int nr_b, PeelBox b, int ntr, int n, int qchunk,
                                                    const double *__restrict__ rec, double *__restrict__ part) {
    extern __shared__ __attribute__((aligned(16))) double seed_sm[];
    double *Z = seed_sm, *rc = seed_sm + 4 * SEED_HN;
    const int tid = threadIdx.x, npix = b.nr * b.nc;
    const int r0 = (int)(blockIdx.x % (unsigned)ntr) * SEED_TILE, c0 = (int)(blockIdx.x / (unsigned)ntr) * SEED_TILE;
    for (int i = tid; i < SEED_HN; i += 256) {
        const int rr = r0 - 1 + i % SEED_HALO, cc = c0 - 1 + i / SEED_HALO;
        const bool inb = rr >= 0 && rr < b.nr && cc >= 0 && cc < b.nc;
        for (int j = 0; j < 3; ++j) rc[i * 3 + j] = inb ? rec[((int64_t)cc * b.nr + rr) * 3 + j] : 0.0;
    }
    const int nq = (n + 3) / 4;
    const int q0 = (int)blockIdx.y * qchunk, q1 = min(nq, q0 + qchunk);
    const int tr = tid & (SEED_TILE - 1), tc = tid / SEED_TILE;
    const bool mine = r0 + tr < b.nr && c0 + tc < b.nc;
    const int ctr = (tc + 1) * SEED_HALO + tr + 1;
    double acc = 0;
    for (int q = q0; q < q1; ++q) {
        __syncthreads();
        for (int i = tid; i < SEED_HN; i += 256) {
            const int rr = r0 - 1 + i % SEED_HALO, cc = c0 - 1 + i / SEED_HALO;
            double z[4] = {0.0, 0.0, 0.0, 0.0};
            if (rr >= 0 && rr < b.nr && cc >= 0 && cc < b.nc) {
                const float4 v4 = hy4[(int64_t)q * d_b + (int64_t)(b.c0 + cc) * nr_b + b.r0 + rr];
                const float v[4] = {v4.x, v4.y, v4.z, v4.w};
                const double *o = rc + i * 3;
#pragma unroll
                for (int j = 0; j < 4; ++j)
                    if (4 * q + j < n) { const double hv = (double)v[j]; z[j] = ((hv < o[0] ? 0.0 : hv) - o[1]) * o[2]; }
            }
#pragma unroll
            for (int j = 0; j < 4; ++j) Z[j * SEED_HN + i] = z[j];
        }
        __syncthreads();
        if (mine) {
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const double *zc = Z + j * SEED_HN + ctr;
                const double nb = ((zc[-SEED_HALO - 1] + zc[-SEED_HALO]) + (zc[-SEED_HALO + 1] + zc[-1])) + ((zc[1] + zc[SEED_HALO - 1]) + (zc[SEED_HALO] + zc[SEED_HALO + 1]));
                acc = fma(zc[0], nb, acc);
            }
        }
    }
    if (mine) part[(int64_t)blockIdx.y * npix + (int64_t)(c0 + tc) * b.nr + r0 + tr] = acc;
}

// tmp_Cn (:400-401): the chunks in ascending order, / n / the neighbours inside the box; NaN or < min_corr -> 0
__global__ void __launch_bounds__(256) k_peel_cn(const double *__restrict__ part, PeelBox b, int nsplit, int n, double min_corr, float *__restrict__ cn) {
    const int i = (int)blockIdx.x * 256 + threadIdx.x, npix = b.nr * b.nc;
    if (i >= npix) return;
    const int r = i % b.nr, c = i / b.nr;
    double s = 0;
    for (int k = 0; k < nsplit; ++k) s += part[(int64_t)k * npix + i];
    const int cnt = (min(r + 1, b.nr - 1) - max(r - 1, 0) + 1) * (min(c + 1, b.nc - 1) - max(c - 1, 0) + 1) - 1;
    const double v = s / (double)n / (double)cnt;
    cn[i] = (v != v || v < min_corr) ? 0.f : (float)v;
}

// ---- host side ---------------------------------------------------------------------------------------------------------------------------------------------
static inline PeelBox peel_box(const PeelSession *S, int r, int c, int reach) {
    PeelBox b;
    b.r0 = std::max(0, r - reach); b.c0 = std::max(0, c - reach);
    b.nr = std::min(S->nr - 1, r + reach) - b.r0 + 1; b.nc = std::min(S->nc - 1, c + reach) - b.c0 + 1;
    return b;
}
static inline void peel_chunks(int64_t nq, int &nch, int &qchunk) {
    nch = (int)std::min<int64_t>(PEEL_NCH, std::max<int64_t>(1, nq / 8));
    qchunk = (int)((nq + nch - 1) / nch);
    nch = (int)((nq + qchunk - 1) / qchunk);
}
static inline size_t peel_al(size_t b) { return (b + 255) & ~size_t(255); }

int peel_open_run(cnmfe_ctx *ctx, Patch *P, const float *psf, int32_t psf_n, int64_t nframes, const double *Q, int32_t M, float sig,
                  float *Cn_out, float *PNR_out, float *Sn_out) {
    PeelSession *S = P->peel;
    const int64_t n = nframes, d_b = P->d_b, nq = (n + 3) / 4;
    S->n = n; S->nq = nq; S->M = M; S->d = d_b; S->nr = P->nr_b; S->nc = P->nc_b; S->residual = false;
    const size_t vid = (size_t)nq * (size_t)d_b * sizeof(float4);
    if (S->hy.ensure(vid) != 0 || S->yw.ensure(vid) != 0) {
        (void)hipGetLastError();
        return fail(CNMFE_ENOMEM, "peel session: no room for the filtered block and the working copy, 2 x %zu bytes (16 x ceil(nframes / 4) x d_b)", vid);
    }
    RET(S->sn.ensure((size_t)d_b * sizeof(double)));
    RET(S->ci.ensure(peel_al((size_t)n * sizeof(double)) * 2));
    RET(seed_images_run(ctx, SeedSrc{P->Yc4.as<float4>(), d_b, P->nr_b, P->nc_b}, psf, psf_n, nframes, Q, M, sig, Cn_out, PNR_out, S));
    if (M > 0) {
        RET(S->q.ensure((size_t)n * M * sizeof(double)));
        CK(hipMemcpyAsync(S->q.p, Q, (size_t)n * M * sizeof(double), hipMemcpyHostToDevice, ctx->st()));
        LAUNCH(ctx, "peel_yw_detrend", k_peel_yw_detrend, dim3((unsigned)d_b), dim3(256), 0, P->Yc4.as<float4>(), S->yw.as<float4>(), d_b, (int)n, S->q.as<double>(), (int)M);
    } else {
        CK(hipMemcpyAsync(S->yw.p, P->Yc4.p, vid, hipMemcpyDeviceToDevice, ctx->st()));
    }
    if (Sn_out) {
        std::vector<double> sn((size_t)d_b);
        CK(hipMemcpyAsync(sn.data(), S->sn.p, (size_t)d_b * sizeof(double), hipMemcpyDeviceToHost, ctx->st()));
        CK(hipStreamSynchronize(ctx->st()));
        for (int64_t i = 0; i < d_b; ++i) Sn_out[i] = (float)sn[(size_t)i];
    }
    CK(hipStreamSynchronize(ctx->st()));                     // (Q is the caller's pageable memory)
    return 0;
}

// The session of the second pass on the PATCH and its residual video (all frames, no detrending: initComponents_residual_parallel.m:176-177,220).
// lowrank = false (cnmfe_peel_open_residual): Yres = Ysig - A C; the caller has made sure that P->ysig holds the residual itself (residual_materialize).
// lowrank = true  (cnmfe_peel_open_lowrank): Yres = Yc + (ymean - b0) - b f - A C from the centred block video and the patch's fp64 factors; P->ysig and the
// residual state are neither read nor written, so the session keeps the state as it found it (PeelSession::keep_resid).
static int peel_open_patch_run(cnmfe_ctx *ctx, Patch *P, bool lowrank, int32_t Ksel, const int64_t *A_colptr, const int32_t *A_rowidx, const float *A_val, const float *C,
                               int c_order, const float *psf, int32_t psf_n, float sig, float *Cn_out, float *PNR_out, float *Sn_out, float *Yres_out, int out_memspace) {
    PeelSession *S = P->peel;
    const int64_t n = P->T, d = P->d, nq = (n + 3) / 4;
    S->n = n; S->nq = nq; S->M = 0; S->d = d; S->nr = P->nr; S->nc = P->nc; S->residual = true; S->keep_resid = lowrank;
    const size_t vid = (size_t)nq * (size_t)d * sizeof(float4);
    if (S->hy.ensure(vid) != 0 || S->yw.ensure(vid) != 0) {
        (void)hipGetLastError();
        return fail(CNMFE_ENOMEM, "residual peel session: no room for the filtered residual video and the working copy, 2 x %zu bytes (16 x ceil(T / 4) x d)", vid);
    }
    RET(S->sn.ensure((size_t)d * sizeof(double)));
    RET(S->ci.ensure(peel_al((size_t)n * sizeof(double)) * 2));
    // (buffers of this call: released when it returns, behind the stream's last wait)
    DevBuf dC, dRow, dCol, dVal;
    int64_t ldc = 4;
    const bool has_ac = Ksel > 0 && A_colptr[Ksel] > 0;
    if (has_ac) {
        RET(upload_traces(ctx, dC, C, Ksel, n, c_order, &ldc));
        HostCSR csr; csc_to_csr(d, Ksel, A_colptr, A_rowidx, A_val, csr);
        RET(to_dev(ctx, dRow, csr.rowptr.data(), csr.rowptr.size()));
        RET(to_dev(ctx, dCol, csr.col.data(), csr.col.size()));
        RET(to_dev(ctx, dVal, csr.val.data(), csr.val.size()));
    }
    // a patch of few pixels splits its frames over workgroups (some thousands wanted); every (pixel, quad) is written by exactly one thread
    const int64_t nblk = (d + 255) / 256;
    int64_t nseg = std::max<int64_t>(1, std::min<int64_t>(nq, (4096 + nblk - 1) / nblk));
    const int qchunk = (int)((nq + nseg - 1) / nseg);
    nseg = (nq + qchunk - 1) / qchunk;
    if (lowrank)
        LAUNCH(ctx, "peel_yres_lowrank", k_peel_yres_lowrank, dim3((unsigned)nblk, (unsigned)nseg), dim3(256), 0, P->Yc4.as<float4>(), P->ymean_f.as<float>(),
               P->svd_b0.as<double>(), P->svd_b.as<double>(), P->svd_f.as<double>(), P->svd_nb, d, P->d_b, (int)n, P->nr, P->nr_b, P->roff, P->coff, qchunk,
               has_ac ? dRow.as<int>() : (const int *)nullptr, dCol.as<int>(), dVal.as<float>(), dC.as<float>(), ldc, S->yw.as<float4>());
    else
        LAUNCH(ctx, "peel_yres", k_peel_yres, dim3((unsigned)nblk, (unsigned)nseg), dim3(256), 0, P->ysig.as<float4>(), d, (int)n, qchunk,
               has_ac ? dRow.as<int>() : (const int *)nullptr, dCol.as<int>(), dVal.as<float>(), dC.as<float>(), ldc, S->yw.as<float4>());
    RET(seed_images_run(ctx, SeedSrc{S->yw.as<float4>(), d, P->nr, P->nc}, psf, psf_n, n, nullptr, 0, sig, Cn_out, PNR_out, S));
    if (Sn_out) {
        std::vector<double> sn((size_t)d);
        CK(hipMemcpyAsync(sn.data(), S->sn.p, (size_t)d * sizeof(double), hipMemcpyDeviceToHost, ctx->st()));
        CK(hipStreamSynchronize(ctx->st()));
        for (int64_t i = 0; i < d; ++i) Sn_out[i] = (float)sn[(size_t)i];
    }
    if (Yres_out) RET(ysig_export(ctx, P, S->yw, Yres_out, out_memspace));      // (nothing has been peeled yet: Yw is Yres) exactly the fp32 video the session searches, frame-major like cnmfe_residual's output
    CK(hipStreamSynchronize(ctx->st()));
    return 0;
}
int peel_open_residual_run(cnmfe_ctx *ctx, Patch *P, int32_t Ksel, const int64_t *A_colptr, const int32_t *A_rowidx, const float *A_val, const float *C, int c_order,
                           const float *psf, int32_t psf_n, float sig, float *Cn_out, float *PNR_out, float *Sn_out, float *Yres_out, int out_memspace) {
    return peel_open_patch_run(ctx, P, false, Ksel, A_colptr, A_rowidx, A_val, C, c_order, psf, psf_n, sig, Cn_out, PNR_out, Sn_out, Yres_out, out_memspace);
}
int peel_open_lowrank_run(cnmfe_ctx *ctx, Patch *P, int32_t Ksel, const int64_t *A_colptr, const int32_t *A_rowidx, const float *A_val, const float *C, int c_order,
                          const float *psf, int32_t psf_n, float sig, float *Cn_out, float *PNR_out, float *Sn_out, float *Yres_out, int out_memspace) {
    return peel_open_patch_run(ctx, P, true, Ksel, A_colptr, A_rowidx, A_val, C, c_order, psf, psf_n, sig, Cn_out, PNR_out, Sn_out, Yres_out, out_memspace);
}

int peel_extract_run(cnmfe_ctx *ctx, Patch *P, int r, int c, int gSiz, double *corr_box, double *ai_box, double *ci_out, double *stats) {
    PeelSession *S = P->peel;
    const int64_t n = S->n, d_b = S->d, nq = S->nq;
    const int nr_b = S->nr;
    const PeelBox b = peel_box(S, r, c, gSiz);
    const int npix = b.nr * b.nc, ictr = (c - b.c0) * b.nr + (r - b.r0);
    const int64_t pctr = (int64_t)c * nr_b + r;
    int nch, qchunk;
    peel_chunks(nq, nch, qchunk);
    const int npart = nch * PEEL_QL;
    WelchPlan w;
    RET(welch_cfg(ctx, n, w));
    float *tabs;
    RET(welch_tabs(ctx, w, 1, &tabs));
    const size_t o_part = 0, o_corr = o_part + peel_al((size_t)npart * npix * 3 * sizeof(double)), o_ai = o_corr + peel_al((size_t)npix * sizeof(double)),
                 o_hi = o_ai + peel_al((size_t)npix * sizeof(double)), o_lo = o_hi + peel_al((size_t)npix * sizeof(int)), o_cnt = o_lo + peel_al((size_t)npix * sizeof(int)),
                 o_mom = o_cnt + 256, o_st = o_mom + 256, total = o_st + 256;
    RET(S->scr.ensure(total));
    char *sb = S->scr.as<char>();
    double *dPart = reinterpret_cast<double *>(sb + o_part), *dCorr = reinterpret_cast<double *>(sb + o_corr), *dAi = reinterpret_cast<double *>(sb + o_ai);
    int *dHi = reinterpret_cast<int *>(sb + o_hi), *dLo = reinterpret_cast<int *>(sb + o_lo), *dCnt = reinterpret_cast<int *>(sb + o_cnt);
    double *dMom = reinterpret_cast<double *>(sb + o_mom), *dSt = reinterpret_cast<double *>(sb + o_st);
    double *dCi = S->ci.as<double>(), *dBg = reinterpret_cast<double *>(S->ci.as<char>() + peel_al((size_t)n * sizeof(double)));
    const float4 *hy4 = S->hy.as<float4>(), *yw4 = S->yw.as<float4>();
    LAUNCH(ctx, "peel_corr_part", k_peel_corr_part, dim3((unsigned)b.nc, (unsigned)nch), dim3(256), 0, hy4, d_b, nr_b, b, pctr, (int)n, qchunk, dPart);
    LAUNCH(ctx, "peel_corr_fin", k_peel_corr_fin, dim3(1), dim3(256), 0, dPart, npart, npix, ictr, (int)n, dCorr, dHi, dLo, dCnt);
    const size_t sh_tr = (size_t)4 * npix * sizeof(double) + 264 * sizeof(int);
    LAUNCH(ctx, "peel_traces", k_peel_traces, dim3((unsigned)nq), dim3(256), sh_tr, hy4, yw4, (S->M > 0 || S->residual || S->no_mean) ? (const double *)nullptr : (S->own_mean ? S->ymean.as<double>() : P->ymean_d.as<double>()), d_b, nr_b, b,
           dHi, dLo, dCnt, (int)n, dCi, dBg);
    if (w.lng) {
        WELCH_LAUNCH_LONG(ctx, "peel_trace_stats", k_peel_trace_stats_long, w, 1, tabs, hy4, d_b, pctr, (const double *)dCi, (const double *)dBg, (const int *)dCnt, dMom, dSt);
    } else {
        if (w.shmem > 64 * 1024) CK(hipFuncSetAttribute((const void *)k_peel_trace_stats, hipFuncAttributeMaxDynamicSharedMemorySize, (int)w.shmem));
        LAUNCH(ctx, "peel_trace_stats", k_peel_trace_stats, dim3(1), dim3(256), w.shmem, w.c, hy4, d_b, pctr, dCi, dBg, dCnt, dMom, dSt);
    }
    LAUNCH(ctx, "peel_mom_part", k_peel_mom_part, dim3((unsigned)b.nc, (unsigned)nch), dim3(256), 0, yw4, d_b, nr_b, b, dCi, dBg, dMom, (int)n, qchunk, dPart);
    LAUNCH(ctx, "peel_ai_fin", k_peel_ai_fin, dim3((unsigned)((npix + 255) / 256)), dim3(256), 0, dPart, npart, npix, dMom, dAi);
    CK(hipMemcpyAsync(corr_box, dCorr, (size_t)npix * sizeof(double), hipMemcpyDeviceToHost, ctx->st()));
    CK(hipMemcpyAsync(ai_box, dAi, (size_t)npix * sizeof(double), hipMemcpyDeviceToHost, ctx->st()));
    CK(hipMemcpyAsync(ci_out, dCi, (size_t)n * sizeof(double), hipMemcpyDeviceToHost, ctx->st()));
    CK(hipMemcpyAsync(stats, dSt, 6 * sizeof(double), hipMemcpyDeviceToHost, ctx->st()));
    CK(hipStreamSynchronize(ctx->st()));
    return 0;
}

int peel_apply_run(cnmfe_ctx *ctx, Patch *P, int r, int c, int gSiz, const double *ai_box, const double *Hai_box2, const double *ci, double sig, double min_pnr,
                   double min_corr, float *PNR_box2, float *Cn_box2) {
    PeelSession *S = P->peel;
    const int64_t n = S->n, d_b = S->d, nq = S->nq;
    const int nr_b = S->nr;
    const PeelBox b = peel_box(S, r, c, gSiz), b2 = peel_box(S, r, c, 2 * gSiz);
    const int npix = b.nr * b.nc, npix2 = b2.nr * b2.nc;
    int nch, qchunk;
    peel_chunks(nq, nch, qchunk);
    const int npart = nch * PEEL_QL;
    const int ntr = (b2.nr + SEED_TILE - 1) / SEED_TILE, ntc = (b2.nc + SEED_TILE - 1) / SEED_TILE;
    const size_t o_part = 0, o_a = o_part + peel_al((size_t)npart * npix2 * 3 * sizeof(double)), o_h = o_a + peel_al((size_t)npix * sizeof(double)),
                 o_rec = o_h + peel_al((size_t)npix2 * sizeof(double)), o_pnr = o_rec + peel_al((size_t)npix2 * 3 * sizeof(double)),
                 o_cn = o_pnr + peel_al((size_t)npix2 * sizeof(float)), total = o_cn + peel_al((size_t)npix2 * sizeof(float));
    RET(S->scr.ensure(total));
    char *sb = S->scr.as<char>();
    double *dPart = reinterpret_cast<double *>(sb + o_part), *dA = reinterpret_cast<double *>(sb + o_a), *dH = reinterpret_cast<double *>(sb + o_h),
           *dRec = reinterpret_cast<double *>(sb + o_rec);
    float *dPnr = reinterpret_cast<float *>(sb + o_pnr), *dCn = reinterpret_cast<float *>(sb + o_cn);
    double *dCi = S->ci.as<double>();
    CK(hipMemcpyAsync(dA, ai_box, (size_t)npix * sizeof(double), hipMemcpyHostToDevice, ctx->st()));
    CK(hipMemcpyAsync(dH, Hai_box2, (size_t)npix2 * sizeof(double), hipMemcpyHostToDevice, ctx->st()));
    CK(hipMemcpyAsync(dCi, ci, (size_t)n * sizeof(double), hipMemcpyHostToDevice, ctx->st()));
    float4 *hy4 = S->hy.as<float4>();
    LAUNCH(ctx, "peel_rank1_yw", k_peel_rank1, dim3((unsigned)b.nc, (unsigned)nch), dim3(256), 0, S->yw.as<float4>(), d_b, nr_b, b, dA, dCi, (int)n, qchunk);
    LAUNCH(ctx, "peel_rank1_hy", k_peel_rank1, dim3((unsigned)b2.nc, (unsigned)nch), dim3(256), 0, hy4, d_b, nr_b, b2, dH, dCi, (int)n, qchunk);
    LAUNCH(ctx, "peel_box_part", k_peel_box_part, dim3((unsigned)b2.nc, (unsigned)nch), dim3(256), 0, hy4, d_b, nr_b, b2, S->sn.as<double>(), sig, (int)n, qchunk, dPart);
    LAUNCH(ctx, "peel_box_rec", k_peel_box_rec, dim3((unsigned)((npix2 + 255) / 256)), dim3(256), 0, dPart, npart, b2, nr_b, S->sn.as<double>(), sig, min_pnr, (int)n,
           dRec, dPnr);
    const size_t sh_corr = ((size_t)4 * SEED_HN + (size_t)SEED_HN * 3) * sizeof(double);
    LAUNCH(ctx, "peel_corr8", k_peel_corr8, dim3((unsigned)(ntr * ntc), (unsigned)nch), dim3(256), sh_corr, hy4, d_b, nr_b, b2, ntr, (int)n, qchunk, dRec, dPart);
    LAUNCH(ctx, "peel_cn", k_peel_cn, dim3((unsigned)((npix2 + 255) / 256)), dim3(256), 0, dPart, b2, nch, (int)n, min_corr, dCn);
    CK(hipMemcpyAsync(PNR_box2, dPnr, (size_t)npix2 * sizeof(float), hipMemcpyDeviceToHost, ctx->st()));
    CK(hipMemcpyAsync(Cn_box2, dCn, (size_t)npix2 * sizeof(float), hipMemcpyDeviceToHost, ctx->st()));
    CK(hipStreamSynchronize(ctx->st()));
    return 0;
}

}  // namespace cnmfe
