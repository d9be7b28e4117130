// (f) seed images: [Cn, PNR] of one block, the data-parallel half of greedyROI_endoscope
//   @Sources2D/correlation_pnr_parallel.m:70-104  ->  endoscope/correlation_image_endoscope.m:36-96  ->  utilities/correlation_image.m:31-77
//   (nk > 1: endoscope/detrend_data.m:22-29 first -- a projection in time, it commutes with the spatial filter and is applied to the filtered trace)
// Included by deconv.hip below get_sn (the noise of the filtered trace is the same Welch estimator).  Three passes over the block:
//   k_seed_filter   HY = imfilter(Y, psf, 'replicate') of the centred video, 4 frames at a time        reads Yc4 once (+ halo), writes HY4 once
//   k_seed_stats    per pixel: detrend, median, max, GetSn, the 3 Sn threshold, mean and rms           reads HY4 once
//                   (k_seed_stats: trace | Welch transform in one workgroup's LDS, up to 20416 frames; k_seed_stats_long beyond, up to WELCH_TMAX = 147456:
//                   the trace in a scratch row of global memory -- at most 1024 rows of ceil4(n) floats, 256 from nfft = 16384 on -- and LDS the transform alone)
//   k_seed_corr     Z = the thresholded, standardised traces rebuilt on the fly; sum_t Z_p sum_N8 Z_n   reads HY4 once (+ 1-pixel halo)
//   k_seed_cn       the partial sums of the frame chunks in a fixed order, / nframes / |N8|
// The pixel mean the resident video lacks is a constant per pixel after the filter: it leaves with the median (and lies in the span of the splines).
#pragma once

namespace cnmfe {

constexpr int SEED_TILE = 16;                         // pixel tile of the filter and the correlation pass: 16 rows x 16 columns, one thread each
constexpr int SEED_MMAX = 16;                         // detrend basis columns
constexpr int SEED_PSF_MAX = 25;                      // filter size (reach 12: a 40 x 40 float4 tile, 25.6 KB of LDS)
constexpr int SEED_REC = 4;                           // per-pixel record: threshold sig * Sn, mean, 1 / rms, median, then the M detrend coefficients (doubles)
constexpr int SEED_HALO = SEED_TILE + 2;              // correlation tile with its 1-pixel halo
constexpr int SEED_HN = SEED_HALO * SEED_HALO;

// y - sum_m a_m Q(t, m) in fp64, rounded once: the ONE form both k_seed_stats (which thresholds the result) and k_seed_corr (which rebuilds it) evaluate, every
// product-sum an explicit fma so that the two kernels cannot be contracted differently
__device__ __forceinline__ float seed_detrend(float y, const double *a, const double *Qt, int64_t n, int M) {
    double s = (double)y;
    for (int m = 0; m < M; ++m) s = fma(-a[m], Qt[(int64_t)m * n], s);
    return (float)s;
}

// One workgroup per (pixel tile, frame quad).  The tile and the filter's reach are staged in LDS with the coordinates clamped to the BLOCK (imfilter 'replicate',
// correlation_image_endoscope.m:79); taps = the non-zero entries of psf in column-major order as (LDS offset from the pixel, weight bits).
__global__ void __launch_bounds__(256) k_seed_filter(const float4 *__restrict__ yc4, int64_t d_b, int nr_b, int nc_b, int ntr, int R,
                                                     const int2 *__restrict__ taps, int ntap, float4 *__restrict__ hy4) {
    extern __shared__ __attribute__((aligned(16))) float4 seed_tile[];
    const int tid = threadIdx.x, W = SEED_TILE + 2 * R;
    const int r0 = (int)(blockIdx.x % (unsigned)ntr) * SEED_TILE, c0 = (int)(blockIdx.x / (unsigned)ntr) * SEED_TILE;
    const float4 *src = yc4 + (int64_t)blockIdx.y * d_b;
    for (int i = tid; i < W * W; i += 256) {
        const int rr = min(max(r0 - R + i % W, 0), nr_b - 1), cc = min(max(c0 - R + i / W, 0), nc_b - 1);
        seed_tile[i] = src[(int64_t)cc * nr_b + rr];
    }
    __syncthreads();
    const int tr = tid & (SEED_TILE - 1), tc = tid / SEED_TILE;
    const int r = r0 + tr, c = c0 + tc;
    if (r >= nr_b || c >= nc_b) return;
    const float4 *ctr = seed_tile + (tc + R) * W + tr + R;
    float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
    for (int k = 0; k < ntap; ++k) {
        const int2 tp = taps[k];
        const float w = __int_as_float(tp.y);
        const float4 v = ctr[tp.x];
        acc.x = fmaf(w, v.x, acc.x); acc.y = fmaf(w, v.y, acc.y); acc.z = fmaf(w, v.z, acc.z); acc.w = fmaf(w, v.w, acc.w);
    }
    hy4[(int64_t)blockIdx.y * d_b + (int64_t)c * nr_b + r] = acc;
}

__device__ __forceinline__ float seed_block_max(float v, double *red) {
    const int tid = threadIdx.x;
    for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o));
    __syncthreads();
    if ((tid & 63) == 0) red[tid >> 6] = (double)v;
    __syncthreads();
    const float r = fmaxf(fmaxf((float)red[0], (float)red[1]), fmaxf((float)red[2], (float)red[3]));
    __syncthreads();
    return r;
}

// One workgroup per block pixel, the LDS layout of k_sn_video: the filtered trace of frames [0, n) | the Welch transform.  Only t < n is ever read: the padding
// frames of the last quad enter nothing.
__global__ void __launch_bounds__(256) k_seed_stats(DeconvCfg c, const float4 *__restrict__ hy4, int64_t d_b, const double *__restrict__ Q, int M, double sig,
                                                    double *__restrict__ rec, float *__restrict__ pnr, double *__restrict__ sn_keep) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    __shared__ double red[4];
    const int64_t p = blockIdx.x;
    const int tid = threadIdx.x, n = c.T;
    const int Tal = (n + 3) & ~3;
    float *y = lds, *scr = lds + Tal;
    // the detrend coefficients and the selection's histogram live in the transform's scratch (at least 640 floats), which get_sn only takes over after them:
    // beside `red` the kernel has no static LDS, so the frame limit is k_sn_video's
    double *coef = reinterpret_cast<double *>(scr);
    int *hist = reinterpret_cast<int *>(scr + 2 * SEED_MMAX);
    double *orec = rec + p * (int64_t)(SEED_REC + M);
    for (int i = tid; i < Tal / 4; i += 256) *reinterpret_cast<float4 *>(y + 4 * i) = hy4[(int64_t)i * d_b + p];
    __syncthreads();
    if (M > 0) {                                             // detrend_data.m:26-29 against an orthonormal basis of the same span: R = Y Q, Ydt = Y - R Q'
        for (int m = 0; m < M; ++m) {
            double s = 0;
            for (int t = tid; t < n; t += 256) s = fma(Q[(int64_t)m * n + t], (double)y[t], s);
            s = block_sum(s, red);
            if (tid == 0) { coef[m] = s; orec[SEED_REC + m] = s; }
        }
        __syncthreads();
        for (int t = tid; t < n; t += 256) y[t] = seed_detrend(y[t], coef, Q + t, n, M);
        __syncthreads();
    }
    float vk, vk1;                                           // median(HY, 2): the middle value, or the mean of the two middle ones (correlation_image_endoscope.m:85)
    select_pair(y, n, (n - 1) / 2, hist, vk, vk1);
    const float med = (n & 1) ? vk : (float)(0.5 * ((double)vk + (double)vk1));
    float mx = -INFINITY;
    __syncthreads();
    for (int t = tid; t < n; t += 256) { const float v = y[t] - med; y[t] = v; mx = fmaxf(mx, v); }
    mx = seed_block_max(mx, red);                            // HY_max (:86); its barriers also publish the median-subtracted trace
    const double sn = get_sn(y, c, scr, red, false);         // Ysig = GetSn(HY) (:87)
    const double thr = sig * sn;                             // HY(HY < Ysig * sig) = 0 (:93)
    double s = 0;
    for (int t = tid; t < n; t += 256) { const double v = (double)y[t]; s += v < thr ? 0.0 : v; }
    const double mean = block_sum(s, red) / (double)n;       // correlation_image.m:32
    s = 0;
    for (int t = tid; t < n; t += 256) { const double v = (double)y[t]; const double x = (v < thr ? 0.0 : v) - mean; s = fma(x, x, s); }
    const double rms = sqrt(block_sum(s, red) / (double)n);  // :47-48
    if (tid == 0) {
        orec[0] = thr; orec[1] = mean; orec[2] = rms == 0.0 ? 1.0 : 1.0 / rms; orec[3] = (double)med;
        pnr[p] = (float)((double)mx / sn);                   // :88
        if (sn_keep) sn_keep[p] = sn;                        // (a peel session keeps Ysig, greedyROI_endoscope.m:132)
    }
}

// The long flavour (welch_cfg, deconv.hip: the trace and the transform do not share 160 KB of LDS, or option trace_long): a workgroup walks the pixels
// blockIdx.x, blockIdx.x + gridDim.x, ... and keeps the trace of the one it is at in ITS row of `rows` (ceil4(n) floats of global memory, filled by one strided
// pass over hy4; every later pass -- the detrend, the selection's histograms, the overlapped Welch segments, the statistics -- reads contiguous memory no other
// workgroup touches).  LDS holds the transform alone, the coefficients and the histogram are static.  Same 256 threads, strides, fma order and (below the split
// tier) get_sn instantiation as k_seed_stats: at a frame count both take, their outputs are equal bit for bit.
template <bool SPLIT>
__global__ void __launch_bounds__(256) k_seed_stats_long(DeconvCfg c, float *__restrict__ tabs, const float4 *__restrict__ hy4, int64_t d_b, const double *__restrict__ Q,
                                                         int M, double sig, float *__restrict__ rows, double *__restrict__ rec, float *__restrict__ pnr,
                                                         double *__restrict__ sn_keep) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    __shared__ double red[4];
    __shared__ double coef[SEED_MMAX];
    __shared__ int hist[260];
    const int tid = threadIdx.x, n = c.T;
    const int Tal = (n + 3) & ~3;
    float *y = rows + (int64_t)blockIdx.x * Tal;
    for (int64_t p = blockIdx.x; p < d_b; p += gridDim.x) {
        double *orec = rec + p * (int64_t)(SEED_REC + M);
        for (int i = tid; i < Tal / 4; i += 256) *reinterpret_cast<float4 *>(y + 4 * i) = hy4[(int64_t)i * d_b + p];
        __threadfence_block();                               // (the row is written and read by this workgroup alone; the barriers order it)
        __syncthreads();
        if (M > 0) {
            for (int m = 0; m < M; ++m) {
                double s = 0;
                for (int t = tid; t < n; t += 256) s = fma(Q[(int64_t)m * n + t], (double)y[t], s);
                s = block_sum(s, red);
                if (tid == 0) { coef[m] = s; orec[SEED_REC + m] = s; }
            }
            __syncthreads();
            for (int t = tid; t < n; t += 256) y[t] = seed_detrend(y[t], coef, Q + t, n, M);
            __threadfence_block();
            __syncthreads();
        }
        float vk, vk1;
        select_pair(y, n, (n - 1) / 2, hist, vk, vk1);
        const float med = (n & 1) ? vk : (float)(0.5 * ((double)vk + (double)vk1));
        float mx = -INFINITY;
        __syncthreads();
        for (int t = tid; t < n; t += 256) { const float v = y[t] - med; y[t] = v; mx = fmaxf(mx, v); }
        __threadfence_block();
        mx = seed_block_max(mx, red);
        const double sn = get_sn_long<SPLIT>(y, c, lds, red, tabs);
        const double thr = sig * sn;
        double s = 0;
        for (int t = tid; t < n; t += 256) { const double v = (double)y[t]; s += v < thr ? 0.0 : v; }
        const double mean = block_sum(s, red) / (double)n;
        s = 0;
        for (int t = tid; t < n; t += 256) { const double v = (double)y[t]; const double x = (v < thr ? 0.0 : v) - mean; s = fma(x, x, s); }
        const double rms = sqrt(block_sum(s, red) / (double)n);
        if (tid == 0) {
            orec[0] = thr; orec[1] = mean; orec[2] = rms == 0.0 ? 1.0 : 1.0 / rms; orec[3] = (double)med;
            pnr[p] = (float)((double)mx / sn);
            if (sn_keep) sn_keep[p] = sn;
        }
        __syncthreads();                                     // (the next pixel overwrites the row and the coefficients)
    }
}

// One workgroup per (pixel tile, frame chunk): the records of the tile and its 1-pixel halo in LDS, then per frame quad Z of those 18 x 18 pixels (0 outside the
// block: imfilter's zero padding, correlation_image.m:75) and Z_p * (sum of the 8 neighbours) added in fp64.  part[chunk][pixel].
__global__ void __launch_bounds__(256) k_seed_corr(const float4 *__restrict__ hy4, int64_t d_b, int nr_b, int nc_b, int ntr, int n, int qchunk,
                                                   const double *__restrict__ Q, int M, const double *__restrict__ rec, double *__restrict__ part) {
    extern __shared__ __attribute__((aligned(16))) double seed_sm[];
    const int recw = SEED_REC + M;
    double *Z = seed_sm, *rc = seed_sm + 4 * SEED_HN;
    const int tid = threadIdx.x;
    const int r0 = (int)(blockIdx.x % (unsigned)ntr) * SEED_TILE, c0 = (int)(blockIdx.x / (unsigned)ntr) * SEED_TILE;
    for (int i = tid; i < SEED_HN; i += 256) {
        const int rr = r0 - 1 + i % SEED_HALO, cc = c0 - 1 + i / SEED_HALO;
        const bool inb = rr >= 0 && rr < nr_b && cc >= 0 && cc < nc_b;
        for (int j = 0; j < recw; ++j) rc[i * recw + j] = inb ? rec[((int64_t)cc * nr_b + rr) * recw + j] : 0.0;
    }
    const int nq = (n + 3) / 4;
    const int q0 = (int)blockIdx.y * qchunk, q1 = min(nq, q0 + qchunk);
    const int tr = tid & (SEED_TILE - 1), tc = tid / SEED_TILE;
    const bool mine = r0 + tr < nr_b && c0 + tc < nc_b;
    const int ctr = (tc + 1) * SEED_HALO + tr + 1;
    double acc = 0;
    for (int q = q0; q < q1; ++q) {
        __syncthreads();                                     // the records are staged / the previous quad's Z has been read
        for (int i = tid; i < SEED_HN; i += 256) {
            const int rr = r0 - 1 + i % SEED_HALO, cc = c0 - 1 + i / SEED_HALO;
            double z[4] = {0.0, 0.0, 0.0, 0.0};
            if (rr >= 0 && rr < nr_b && cc >= 0 && cc < nc_b) {
                const float4 v4 = hy4[(int64_t)q * d_b + (int64_t)cc * nr_b + rr];
                const float v[4] = {v4.x, v4.y, v4.z, v4.w};
                const double *o = rc + i * recw;
                const float med = (float)o[3];
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const int t = 4 * q + j;
                    if (t < n) {                             // (the padding frames of the last quad enter nothing)
                        const float yd = M > 0 ? seed_detrend(v[j], o + SEED_REC, Q + t, n, M) : v[j];
                        const double hv = (double)(yd - med);
                        z[j] = ((hv < o[0] ? 0.0 : hv) - o[1]) * o[2];
                    }
                }
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
    if (mine) part[(int64_t)blockIdx.y * d_b + (int64_t)(c0 + tc) * nr_b + r0 + tr] = acc;
}

// Cn = mean(Yconv .* Y, 3) ./ MASK (correlation_image.m:76-77): the chunks' sums in ascending order, MASK = the 8 neighbours inside the block
__global__ void __launch_bounds__(256) k_seed_cn(const double *__restrict__ part, int64_t d_b, int nr_b, int nc_b, int nsplit, int n, float *__restrict__ cn) {
    const int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (p >= d_b) return;
    const int r = (int)(p % nr_b), c = (int)(p / nr_b);
    double s = 0;
    for (int k = 0; k < nsplit; ++k) s += part[(int64_t)k * d_b + p];
    const int cnt = (min(r + 1, nr_b - 1) - max(r - 1, 0) + 1) * (min(c + 1, nc_b - 1) - max(c - 1, 0) + 1) - 1;
    cn[p] = (float)(s / (double)n / (double)cnt);
}

// HY as greedyROI_endoscope.m:130 holds it, in place; the padding frames of the last quad become 0
__global__ void __launch_bounds__(256) k_peel_hy_final(float4 *__restrict__ hy4, int64_t d_b, int n, const double *__restrict__ Q, int M,
                                                       const double *__restrict__ rec) {
    const int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (p >= d_b) return;
    const int q = (int)blockIdx.y;
    const double *o = rec + p * (int64_t)(SEED_REC + M);
    const float med = (float)o[3];
    const float4 v4 = hy4[(int64_t)q * d_b + p];
    float v[4] = {v4.x, v4.y, v4.z, v4.w};
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int t = 4 * q + j;
        v[j] = t < n ? (M > 0 ? seed_detrend(v[j], o + SEED_REC, Q + t, n, M) : v[j]) - med : 0.f;
    }
    hy4[(int64_t)q * d_b + p] = make_float4(v[0], v[1], v[2], v[3]);
}

// src: the video and its geometry -- the centred block of a patch (cnmfe_seed_images, cnmfe_peel_open) or the residual video of a patch (cnmfe_peel_open_residual)
int seed_images_run(cnmfe_ctx *ctx, const SeedSrc &src, const float *psf, int32_t psf_n, int64_t nframes, const double *Q, int32_t M, float sig,
                    float *Cn_out, float *PNR_out, PeelSession *keep) {
    const int64_t n = nframes, d_b = src.d;
    const int nr_b = src.nr, nc_b = src.nc;
    const int64_t nq = (n + 3) / 4;
    WelchPlan w;
    RET(welch_cfg(ctx, n, w));
    // everything the call allocates lives in these two and is released when it returns (seeding runs once per recording, the fits want the room): the filtered
    // block, and ONE allocation for all the small arrays -- every hipFree drains the device, and a patched run makes this call once per patch
    // (a peel session -- peel.hpp -- keeps the filtered block and the noise levels: `keep`; the long flavour's trace rows and table slots are the context's
    // deconvolution scratch, which the long deconvolution of the same recording needs at that size anyway)
    DevBuf hy_call, small;
    DevBuf &hy = keep ? keep->hy : hy_call;
    const int ntr = (nr_b + SEED_TILE - 1) / SEED_TILE, ntc = (nc_b + SEED_TILE - 1) / SEED_TILE;
    const int ntile = ntr * ntc;
    const bool filt = psf && psf_n > 0;
    const int R = filt ? psf_n / 2 : 0, W = SEED_TILE + 2 * R;
    std::vector<int2> taps;
    if (filt)
        for (int j = 0; j < psf_n; ++j)
            for (int i = 0; i < psf_n; ++i) {
                const float w = psf[i + (size_t)j * psf_n];
                if (w != 0.f) { int2 tp; tp.x = (j - R) * W + (i - R); memcpy(&tp.y, &w, sizeof(float)); taps.push_back(tp); }
            }
    // a block of few tiles splits its frames over workgroups (two per CU wanted); a chunk is at least 8 quads, and the chunks are summed in ascending order
    int nsplit = (int)std::min<int64_t>((512 + ntile - 1) / ntile, std::max<int64_t>(1, nq / 8));
    const int qchunk = (int)((nq + nsplit - 1) / nsplit);
    nsplit = (int)((nq + qchunk - 1) / qchunk);
    const int recw = SEED_REC + M;
    auto al = [](size_t b) { return (b + 255) & ~size_t(255); };
    const size_t o_rec = 0, o_part = o_rec + al((size_t)d_b * recw * sizeof(double)), o_q = o_part + al((size_t)nsplit * d_b * sizeof(double)),
                 o_taps = o_q + al((size_t)n * M * sizeof(double)), o_pnr = o_taps + al(taps.size() * sizeof(int2)), o_cn = o_pnr + al((size_t)d_b * sizeof(float)),
                 total = o_cn + al((size_t)d_b * sizeof(float));
    RET(small.ensure(total));
    char *sb = small.as<char>();
    double *dRec = reinterpret_cast<double *>(sb + o_rec), *dPart = reinterpret_cast<double *>(sb + o_part), *dQ = M > 0 ? reinterpret_cast<double *>(sb + o_q) : nullptr;
    int2 *dTaps = reinterpret_cast<int2 *>(sb + o_taps);
    float *dPnr = reinterpret_cast<float *>(sb + o_pnr), *dCn = reinterpret_cast<float *>(sb + o_cn);
    if (M > 0) CK(hipMemcpyAsync(dQ, Q, (size_t)n * M * sizeof(double), hipMemcpyHostToDevice, ctx->st()));
    const float4 *hy4 = src.y4;                                 // gSig <= 0: psf = [] (correlation_image_endoscope.m:45-47,80-82), the video itself
    if (filt) {
        const size_t need = (size_t)nq * (size_t)d_b * sizeof(float4);
        if (hy.ensure(need) != 0) {
            (void)hipGetLastError();
            return fail(CNMFE_ENOMEM, "seed images: no room for the filtered block, %zu bytes (16 x ceil(nframes / 4) x d_b = 16 x %lld x %lld) are needed", need, (long long)nq, (long long)d_b);
        }
        if (!taps.empty()) CK(hipMemcpyAsync(dTaps, taps.data(), taps.size() * sizeof(int2), hipMemcpyHostToDevice, ctx->st()));
        CK(hipStreamSynchronize(ctx->st()));                                 // (`taps` is pageable host memory of this frame)
        LAUNCH(ctx, "seed_filter", k_seed_filter, dim3((unsigned)ntile, (unsigned)nq), dim3(256), (size_t)W * W * sizeof(float4),
               src.y4, d_b, nr_b, nc_b, ntr, R, dTaps, (int)taps.size(), hy.as<float4>());
        hy4 = hy.as<float4>();
    }
    double *dSnKeep = keep ? keep->sn.as<double>() : (double *)nullptr;
    if (w.lng) {
        const unsigned nwg = w.nwg(d_b);
        float *tabs;
        RET(welch_tabs(ctx, w, nwg, &tabs));
        RET(ctx->dscr.ybuf.ensure((size_t)nwg * (size_t)(4 * nq) * sizeof(float)));
        WELCH_LAUNCH_LONG(ctx, "seed_stats", k_seed_stats_long, w, nwg, tabs, hy4, d_b, (const double *)dQ, (int)M, (double)sig, ctx->dscr.ybuf.as<float>(), dRec, dPnr, dSnKeep);
    } else {
        if (w.shmem > 64 * 1024) CK(hipFuncSetAttribute((const void *)k_seed_stats, hipFuncAttributeMaxDynamicSharedMemorySize, (int)w.shmem));
        LAUNCH(ctx, "seed_stats", k_seed_stats, dim3((unsigned)d_b), dim3(256), w.shmem, w.c, hy4, d_b, dQ, (int)M, (double)sig, dRec, dPnr, dSnKeep);
    }
    const size_t sh_corr = ((size_t)4 * SEED_HN + (size_t)SEED_HN * recw) * sizeof(double);
    LAUNCH(ctx, "seed_corr", k_seed_corr, dim3((unsigned)ntile, (unsigned)nsplit), dim3(256), sh_corr, hy4, d_b, nr_b, nc_b, ntr, (int)n, qchunk,
           dQ, (int)M, dRec, dPart);
    LAUNCH(ctx, "seed_cn", k_seed_cn, dim3((unsigned)((d_b + 255) / 256)), dim3(256), 0, dPart, d_b, nr_b, nc_b, nsplit, (int)n, dCn);
    if (keep) {                                                              // HY of greedyROI_endoscope.m:130 in place, by the arithmetic of the two kernels above
        if (!filt) CK(hipMemcpyAsync(hy.p, src.y4, (size_t)nq * (size_t)d_b * sizeof(float4), hipMemcpyDeviceToDevice, ctx->st()));
        LAUNCH(ctx, "peel_hy_final", k_peel_hy_final, dim3((unsigned)((d_b + 255) / 256), (unsigned)nq), dim3(256), 0, hy.as<float4>(), d_b, (int)n, dQ, (int)M, dRec);
    }
    CK(hipMemcpyAsync(Cn_out, dCn, (size_t)d_b * sizeof(float), hipMemcpyDeviceToHost, ctx->st()));
    CK(hipMemcpyAsync(PNR_out, dPnr, (size_t)d_b * sizeof(float), hipMemcpyDeviceToHost, ctx->st()));
    CK(hipStreamSynchronize(ctx->st()));
    return 0;
}

}  // namespace cnmfe
