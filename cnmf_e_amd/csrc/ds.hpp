// (g') down-sampled initialisation: Yds = dsData(Y) of a resident block (utilities/dsData.m:29-43), the source video of cnmfe_seed_images_ds and cnmfe_peel_open_ds
//   spatial   per frame imresize(., [ceil(nr / ssub), ceil(nc / ssub)], 'box'): the separable `contributions` rule make_taps (ssub.hip) restates, with the box
//             kernel -0.5 <= x < 0.5 stretched by in / out PER DIMENSION (antialiasing), the taps mirrored at the border, each row of weights normalised
//   temporal  the mean of every tsub consecutive frames, Ts = floor(n / tsub), the rest discarded
// Included by deconv.hip below seed.hpp and peel.hpp (the session's open and the seed pipeline it runs).  The centred video Yc4 is read once and the down-sampled quads are written once:
//   k_ds_video   one thread per (low-resolution pixel, output quad Q); it consumes exactly the input quads [Q tsub, (Q + 1) tsub).  A wave's lanes run along the
//                output rows, so the row taps of neighbouring lanes tile the input column and whole cache lines are used.  Per input frame the taps are summed in
//                fp64 (column taps ascending, row taps ascending inside), the frames of a bin are added in ascending order, the mean is rounded ONCE to fp32.
//   k_ds_coef    (pre-detrending, initComponents_parallel.m:341-343 BEFORE greedyROI_endoscope.m:52) G[m] = sum_t Qpre(t, m) Ys(p, t) over all n frames, Ys the
//                spatially resized pixel formed on the fly; per-thread partial sums over frame chunks, added in ascending chunk order by k_ds_coef_fin.
//                dsData(Y - (Y Q) Q') = dsData(Y) - sum_m mean_bin(Q(:, m)) G[m]: both maps are linear, one acts in space and one in time, so no full-resolution
//                detrended copy exists; k_ds_video subtracts the correction in fp64 before its single rounding.
// Because the box weights sum to 1, dsData(raw) = dsData(Yc) + box(ymean): k_ds_mean resizes the patch's fp64 pixel mean for the session.
// The second pass (cnmfe_peel_open_residual_ds) opens its session on dsData(Yres), Yres = Ysig - A C of the PATCH, by the same linearity:
//   k_ds_video_res     dsData(Ysig) - A_ds C_ds off the resident residual: k_ds_video's layout and bins (DsPix::bins), then the pixel's CSR row of A_ds times the bin means
//                      of the traces in fp64, ONE rounding.  No full-resolution Yres exists.
//   k_trace_bin_mean   C_ds, K x Ts fp64, on the device so that a bound C never comes down.  A_ds is formed on the host in float64: ds_fold.hpp.
#pragma once
#include "ds_fold.hpp"   // the host rules: ds_box_taps, A_ds (ds_fold_csc), the bin mean

namespace cnmfe {

// geometry and tap tables of one call, as the kernels take them
struct DsGeo {
    int64_t d_in, ds; int nr_in, d1s, ntr, ntc;
    const int *ri, *ci; const double *rw, *cw;
};

// one thread's taps in registers (NT is a compile-time bound: the arrays are never indexed at run time)
template <int NT> struct DsPix {
    int offr[NT]; int64_t offc[NT]; double wr[NT], wc[NT];
    __device__ __forceinline__ void load(const DsGeo &g, int64_t p) {
        const int ro = (int)(p % g.d1s), co = (int)(p / g.d1s);
#pragma unroll
        for (int k = 0; k < NT; ++k) {
            const bool r = k < g.ntr, c = k < g.ntc;
            offr[k] = r ? g.ri[ro * g.ntr + k] : 0; wr[k] = r ? g.rw[ro * g.ntr + k] : 0.0;
            offc[k] = c ? (int64_t)g.ci[co * g.ntc + k] * g.nr_in : 0; wc[k] = c ? g.cw[co * g.ntc + k] : 0.0;
        }
    }
    // the resized pixel of the four frames of one input quad
    __device__ __forceinline__ void quad(const DsGeo &g, const float4 *__restrict__ src, double s[4]) const {
        s[0] = s[1] = s[2] = s[3] = 0.0;
#pragma unroll
        for (int kc = 0; kc < NT; ++kc) {
#pragma unroll
            for (int kr = 0; kr < NT; ++kr) {
                if (kc < g.ntc && kr < g.ntr) {              // (uniform: the tap counts are the call's)
                    const double w = wc[kc] * wr[kr];
                    const float4 v = src[offc[kc] + offr[kr]];
                    s[0] = fma(w, (double)v.x, s[0]); s[1] = fma(w, (double)v.y, s[1]); s[2] = fma(w, (double)v.z, s[2]); s[3] = fma(w, (double)v.w, s[3]);
                }
            }
        }
    }
    // the SUMS of the four bins of output quad Q: it consumes exactly the input quads [Q tsub, (Q + 1) tsub), the frames of a bin added in ascending order
    __device__ __forceinline__ void bins(const DsGeo &g, const float4 *__restrict__ src4, int nq_in, int Q, int tsub, double acc[4]) const {
        acc[0] = acc[1] = acc[2] = acc[3] = 0.0;
        for (int lq = 0; lq < tsub; ++lq) {
            const int64_t iq = (int64_t)Q * tsub + lq;
            if (iq >= nq_in) break;                          // (only behind the last output frame: t < Ts reads input frames below Ts tsub <= n)
            double s[4];
            quad(g, src4 + iq * g.d_in, s);
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const int j = (4 * lq + e) / tsub;           // the output frame of the quad this input frame belongs to
#pragma unroll
                for (int jj = 0; jj < 4; ++jj) if (j == jj) acc[jj] += s[e];
            }
        }
    }
};

// grid (ceil(ds / 256), output quads).  G: [M][ds] (k_ds_coef_fin), bm: [M][Ts] the bin means of Qpre's columns; M = 0: no correction.
template <int NT>
__global__ void __launch_bounds__(256) k_ds_video(const float4 *__restrict__ yc4, int nq_in, DsGeo g, int tsub, int Ts, const double *__restrict__ G,
                                                  const double *__restrict__ bm, int M, float4 *__restrict__ out4) {
    const int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (p >= g.ds) return;
    const int Q = (int)blockIdx.y;
    DsPix<NT> px; px.load(g, p);
    double acc[4];
    px.bins(g, yc4, nq_in, Q, tsub, acc);
    float o[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int t = 4 * Q + j;
        double v = 0.0;
        if (t < Ts) {
            v = acc[j] / (double)tsub;
            for (int m = 0; m < M; ++m) v = fma(-bm[(int64_t)m * Ts + t], G[(int64_t)m * g.ds + p], v);
        }
        o[j] = (float)v;                                     // the padding frames of the last quad: 0
    }
    out4[(int64_t)Q * g.ds + p] = make_float4(o[0], o[1], o[2], o[3]);
}

// The source video of the SECOND pass (cnmfe_peel_open_residual_ds): dsData(Ysig - A C) = dsData(Ysig) - A_ds C_ds off the resident residual of the PATCH
// (g: d_in = d, nr_in = nr of the patch).  k_ds_video's thread layout and bins; then the pixel's stored low-resolution footprints (CSR row of A_ds, columns
// ascending; fp64) times the bin means of their traces (cds: [K][Ts] fp64, k_trace_bin_mean) leave in fp64, and the difference is rounded ONCE.  Every
// (pixel, quad) is written by one thread and every sum has one order: no atomics, equal bits between runs.  16 tsub ntr ntc bytes read per thread through whole
// cache lines (the lanes run along the output rows), 16 written; the trace values of a wave's few neurons come from L2 as in k_peel_yres.
// rowptr == nullptr: no footprint in the patch, plain dsData(Ysig).
template <int NT>
__global__ void __launch_bounds__(256) k_ds_video_res(const float4 *__restrict__ ysig4, int nq_in, DsGeo g, int tsub, int Ts, const int *__restrict__ rowptr,
                                                      const int *__restrict__ col, const double *__restrict__ val, const double *__restrict__ cds,
                                                      float4 *__restrict__ out4) {
    const int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (p >= g.ds) return;
    const int Q = (int)blockIdx.y;
    DsPix<NT> px; px.load(g, p);
    double acc[4];
    px.bins(g, ysig4, nq_in, Q, tsub, acc);
    double v[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) v[j] = 4 * Q + j < Ts ? acc[j] / (double)tsub : 0.0;      // the padding frames of the last quad: 0
    const int e0 = rowptr ? rowptr[p] : 0, e1 = rowptr ? rowptr[p + 1] : 0;
    for (int e = e0; e < e1; ++e) {
        const double a = -val[e];
        const double *c = cds + (int64_t)col[e] * Ts + 4 * (int64_t)Q;
#pragma unroll
        for (int j = 0; j < 4; ++j) if (4 * Q + j < Ts) v[j] = fma(a, c[j], v[j]);
    }
    out4[(int64_t)Q * g.ds + p] = make_float4((float)v[0], (float)v[1], (float)v[2], (float)v[3]);
}

// C_ds: the bin means of K traces (rows of stride ldc floats, upload_traces' layout), [K][Ts] fp64.  One thread per (bin, trace): ds_bin_mean (ds_fold.hpp).
__global__ void __launch_bounds__(256) k_trace_bin_mean(const float *__restrict__ C, int64_t ldc, int tsub, int Ts, double *__restrict__ cds) {
    const int t = (int)blockIdx.x * 256 + threadIdx.x, k = (int)blockIdx.y;
    if (t >= Ts) return;
    cds[(int64_t)k * Ts + t] = ds_bin_mean(C + (int64_t)k * ldc + (int64_t)t * tsub, tsub);
}

// grid (ceil(ds / 256), frame chunks): part[(chunk * M + m) * ds + p] = sum over the chunk's frames t < n of Q[m * n + t] Ys(p, t), frames ascending
template <int NT>
__global__ void __launch_bounds__(256) k_ds_coef(const float4 *__restrict__ yc4, DsGeo g, int n, int qchunk, const double *__restrict__ Qp, int M,
                                                 double *__restrict__ part) {
    const int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (p >= g.ds) return;
    const int nq = (n + 3) / 4, q0 = (int)blockIdx.y * qchunk, q1 = min(nq, q0 + qchunk);
    DsPix<NT> px; px.load(g, p);
    double acc[SEED_MMAX];
#pragma unroll
    for (int m = 0; m < SEED_MMAX; ++m) acc[m] = 0.0;
    for (int q = q0; q < q1; ++q) {
        double s[4];
        px.quad(g, yc4 + (int64_t)q * g.d_in, s);
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const int t = 4 * q + e;
            if (t < n) {
#pragma unroll
                for (int m = 0; m < SEED_MMAX; ++m) if (m < M) acc[m] = fma(Qp[(int64_t)m * n + t], s[e], acc[m]);
            }
        }
    }
#pragma unroll
    for (int m = 0; m < SEED_MMAX; ++m) if (m < M) part[((int64_t)blockIdx.y * M + m) * g.ds + p] = acc[m];
}

// G[m * ds + p]: the chunks in ascending order
__global__ void __launch_bounds__(256) k_ds_coef_fin(const double *__restrict__ part, int64_t ds, int M, int nch, double *__restrict__ G) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= ds * M) return;
    double s = 0;
    for (int k = 0; k < nch; ++k) s += part[(int64_t)k * M * ds + i];
    G[i] = s;
}

// box(ymean): the pixel offset of the down-sampled raw video, fp64
__global__ void __launch_bounds__(256) k_ds_mean(const double *__restrict__ ymean, DsGeo g, double *__restrict__ out) {
    const int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (p >= g.ds) return;
    const int ro = (int)(p % g.d1s), co = (int)(p / g.d1s);
    double s = 0;
    for (int kc = 0; kc < g.ntc; ++kc)
        for (int kr = 0; kr < g.ntr; ++kr)
            s = fma(g.cw[co * g.ntc + kc] * g.rw[ro * g.ntr + kr], ymean[(int64_t)g.ci[co * g.ntc + kc] * g.nr_in + g.ri[ro * g.ntr + kr]], s);
    out[p] = s;
}

// the 4-frame interleaved video as the ABI hands videos out: ds x Ts, frame-major
__global__ void __launch_bounds__(256) k_ds_unpack(const float4 *__restrict__ y4, int64_t ds, int Ts, float *__restrict__ dst) {
    const int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (p >= ds) return;
    const int q = (int)blockIdx.y;
    const float4 v4 = y4[(int64_t)q * ds + p];
    const float v[4] = {v4.x, v4.y, v4.z, v4.w};
#pragma unroll
    for (int j = 0; j < 4; ++j) if (4 * q + j < Ts) dst[(int64_t)(4 * q + j) * ds + p] = v[j];
}

// ---- host side ---------------------------------------------------------------------------------------------------------------------------------------------
// what one call holds on the device until its last kernel has run (the caller synchronises before this goes out of scope)
struct DsCall {
    int ssub = 1, tsub = 1, d1s = 0, d2s = 0; int64_t ds = 0, Ts = 0, nq = 0;
    DsGeo g{};
    DevBuf ri, rw, ci, cw, q, bm, G, part;
};

#define DS_LAUNCH_NT(ctx, name, kern, nt, grid, ...) do { \
    if ((nt) <= 1)      LAUNCH(ctx, name, (kern<1>), grid, dim3(256), 0, __VA_ARGS__); \
    else if ((nt) <= 2) LAUNCH(ctx, name, (kern<2>), grid, dim3(256), 0, __VA_ARGS__); \
    else if ((nt) <= 3) LAUNCH(ctx, name, (kern<3>), grid, dim3(256), 0, __VA_ARGS__); \
    else if ((nt) <= 5) LAUNCH(ctx, name, (kern<5>), grid, dim3(256), 0, __VA_ARGS__); \
    else                LAUNCH(ctx, name, (kern<DS_NT_MAX>), grid, dim3(256), 0, __VA_ARGS__); \
} while (0)

// the plan of one call on a source video of nr x nc pixels (d = nr nc float4s per frame quad): the BLOCK for the first pass, the PATCH for the second
static int ds_plan(cnmfe_ctx *ctx, int nr, int nc, int64_t d, int ssub, int tsub, int64_t nframes, DsCall &c, DsTaps *tr_out = nullptr, DsTaps *tc_out = nullptr) {
    c.ssub = ssub; c.tsub = tsub;
    c.d1s = (nr + ssub - 1) / ssub; c.d2s = (nc + ssub - 1) / ssub; c.ds = (int64_t)c.d1s * c.d2s;
    c.Ts = nframes / tsub; c.nq = (c.Ts + 3) / 4;
    const DsTaps tr = ds_box_taps(nr, c.d1s), tc = ds_box_taps(nc, c.d2s);
    if (tr.nt > DS_NT_MAX || tc.nt > DS_NT_MAX) return fail(CNMFE_EUNSUPPORTED, "down-sampling: %d / %d box taps per sample (at most %d)", tr.nt, tc.nt, DS_NT_MAX);
    RET(to_dev(ctx, c.ri, tr.idx)); RET(to_dev(ctx, c.rw, tr.w)); RET(to_dev(ctx, c.ci, tc.idx)); RET(to_dev(ctx, c.cw, tc.w));
    c.g.d_in = d; c.g.ds = c.ds; c.g.nr_in = nr; c.g.d1s = c.d1s; c.g.ntr = tr.nt; c.g.ntc = tc.nt;
    c.g.ri = c.ri.as<int>(); c.g.ci = c.ci.as<int>(); c.g.rw = c.rw.as<double>(); c.g.cw = c.cw.as<double>();
    if (tr_out) *tr_out = tr;
    if (tc_out) *tc_out = tc;
    return 0;
}

// dst (c.nq * c.ds float4, allocated by the caller) = dsData of the centred block, of the pre-detrended one with Mpre > 0 (Qpre: nframes x Mpre, column-major)
static int ds_video_run(cnmfe_ctx *ctx, Patch *P, DsCall &c, int64_t nframes, const double *Qpre, int32_t Mpre, float4 *dst) {
    const int64_t n = nframes, nq_in = (n + 3) / 4;
    const int nt = std::max(c.g.ntr, c.g.ntc);
    const unsigned nblk = (unsigned)((c.ds + 255) / 256);
    if (Mpre > 0) {
        RET(c.q.ensure((size_t)n * Mpre * sizeof(double)));
        CK(hipMemcpyAsync(c.q.p, Qpre, (size_t)n * Mpre * sizeof(double), hipMemcpyHostToDevice, ctx->st()));
        std::vector<double> bm((size_t)c.Ts * Mpre);
        for (int m = 0; m < Mpre; ++m)
            for (int64_t t = 0; t < c.Ts; ++t) {
                double s = 0;
                for (int i = 0; i < c.tsub; ++i) s += Qpre[(size_t)m * n + (size_t)(t * c.tsub + i)];
                bm[(size_t)m * c.Ts + (size_t)t] = s / (double)c.tsub;
            }
        RET(to_dev(ctx, c.bm, bm));
        int nch, qchunk;
        peel_chunks(nq_in, nch, qchunk);
        RET(c.part.ensure((size_t)nch * Mpre * (size_t)c.ds * sizeof(double)));
        RET(c.G.ensure((size_t)Mpre * (size_t)c.ds * sizeof(double)));
        DS_LAUNCH_NT(ctx, "ds_coef", k_ds_coef, nt, dim3(nblk, (unsigned)nch), P->Yc4.as<float4>(), c.g, (int)n, qchunk, c.q.as<double>(), (int)Mpre, c.part.as<double>());
        LAUNCH(ctx, "ds_coef_fin", k_ds_coef_fin, dim3((unsigned)((c.ds * Mpre + 255) / 256)), dim3(256), 0, c.part.as<double>(), c.ds, (int)Mpre, nch, c.G.as<double>());
    }
    DS_LAUNCH_NT(ctx, "ds_video", k_ds_video, nt, dim3(nblk, (unsigned)c.nq), P->Yc4.as<float4>(), (int)nq_in, c.g, c.tsub, (int)c.Ts,
                 Mpre > 0 ? c.G.as<double>() : (const double *)nullptr, Mpre > 0 ? c.bm.as<double>() : (const double *)nullptr, (int)Mpre, dst);
    return 0;
}

// ds x Ts frame-major, to host or device memory
static int ds_export(cnmfe_ctx *ctx, const DsCall &c, const float4 *y4, float *out, int out_memspace) {
    float *dstp = out;
    const size_t bytes = (size_t)c.ds * (size_t)c.Ts * sizeof(float);
    if (out_memspace != CNMFE_DEVICE) { RET(ctx->stage.ensure(bytes)); dstp = ctx->stage.as<float>(); }
    LAUNCH(ctx, "ds_unpack", k_ds_unpack, dim3((unsigned)((c.ds + 255) / 256), (unsigned)c.nq), dim3(256), 0, y4, c.ds, (int)c.Ts, dstp);
    if (out_memspace != CNMFE_DEVICE) CK(hipMemcpyAsync(out, dstp, bytes, hipMemcpyDeviceToHost, ctx->st()));
    CK(hipStreamSynchronize(ctx->st()));
    return 0;
}

// cnmfe_seed_images_ds (correlation_pnr_parallel.m:86-96): down-sample first, then the seed pipeline detrends the SHORT series (Q: Ts x M).  The down-sampled
// video is scratch of the call.
int seed_images_ds_run(cnmfe_ctx *ctx, Patch *P, int ssub, int tsub, const float *psf, int32_t psf_n, int64_t nframes, const double *Q, int32_t M, float sig,
                       float *Cn_out, float *PNR_out) {
    DsCall c;
    RET(ds_plan(ctx, P->nr_b, P->nc_b, P->d_b, ssub, tsub, nframes, c));
    DevBuf yds;
    const size_t vid = (size_t)c.nq * (size_t)c.ds * sizeof(float4);
    if (yds.ensure(vid) != 0) {
        (void)hipGetLastError();
        return fail(CNMFE_ENOMEM, "seed images: no room for the down-sampled block, %zu bytes (16 x ceil(Ts / 4) x d1s d2s = 16 x %lld x %lld) are needed", vid, (long long)c.nq, (long long)c.ds);
    }
    RET(ds_video_run(ctx, P, c, nframes, nullptr, 0, yds.as<float4>()));
    const int rc = seed_images_run(ctx, SeedSrc{yds.as<float4>(), c.ds, c.d1s, c.d2s}, psf, psf_n, c.Ts, Q, M, sig, Cn_out, PNR_out);
    (void)hipStreamSynchronize(ctx->st());                   // (the tables and the video of this frame are read until here)
    return rc;
}

// cnmfe_peel_open_ds: the session on the down-sampled block.  Yw IS the down-sampled video until the first apply (as in the residual session); the seed pipeline
// runs on it with M = 0 (the trend left before the down-sampling: Qpre), and y_bg adds the session's own pixel mean box(ymean) -- none with Mpre > 0, the
// detrended video carries no mean (the ymean == nullptr branch of k_peel_traces, as for M > 0 in cnmfe_peel_open).
int peel_open_ds_run(cnmfe_ctx *ctx, Patch *P, int ssub, int tsub, const float *psf, int32_t psf_n, int64_t nframes, const double *Qpre, int32_t Mpre, float sig,
                     float *Cn_out, float *PNR_out, float *Sn_out, float *Yds_out, int out_memspace) {
    PeelSession *S = P->peel;
    DsCall c;
    RET(ds_plan(ctx, P->nr_b, P->nc_b, P->d_b, ssub, tsub, nframes, c));
    S->n = c.Ts; S->nq = c.nq; S->M = 0; S->d = c.ds; S->nr = c.d1s; S->nc = c.d2s; S->residual = false; S->own_mean = Mpre == 0; S->no_mean = Mpre > 0;
    const size_t vid = (size_t)c.nq * (size_t)c.ds * sizeof(float4);
    if (S->hy.ensure(vid) != 0 || S->yw.ensure(vid) != 0) {
        (void)hipGetLastError();
        return fail(CNMFE_ENOMEM, "down-sampled peel session: no room for the filtered video and the working copy, 2 x %zu bytes (16 x ceil(Ts / 4) x d1s d2s)", vid);
    }
    RET(S->sn.ensure((size_t)c.ds * sizeof(double)));
    RET(S->ci.ensure(peel_al((size_t)c.Ts * sizeof(double)) * 2));
    if (ssub == 1 && tsub == 1 && Mpre == 0) {               // the identity: the copy cnmfe_peel_open makes
        CK(hipMemcpyAsync(S->yw.p, P->Yc4.p, vid, hipMemcpyDeviceToDevice, ctx->st()));
    } else {
        RET(ds_video_run(ctx, P, c, nframes, Qpre, Mpre, S->yw.as<float4>()));
    }
    if (S->own_mean) {
        RET(S->ymean.ensure((size_t)c.ds * sizeof(double)));
        LAUNCH(ctx, "ds_mean", k_ds_mean, dim3((unsigned)((c.ds + 255) / 256)), dim3(256), 0, P->ymean_d.as<double>(), c.g, S->ymean.as<double>());
    }
    RET(seed_images_run(ctx, SeedSrc{S->yw.as<float4>(), c.ds, c.d1s, c.d2s}, psf, psf_n, c.Ts, nullptr, 0, sig, Cn_out, PNR_out, S));
    if (Sn_out) {
        std::vector<double> sn((size_t)c.ds);
        CK(hipMemcpyAsync(sn.data(), S->sn.p, (size_t)c.ds * sizeof(double), hipMemcpyDeviceToHost, ctx->st()));
        CK(hipStreamSynchronize(ctx->st()));
        for (int64_t i = 0; i < c.ds; ++i) Sn_out[i] = (float)sn[(size_t)i];
    }
    if (Yds_out) RET(ds_export(ctx, c, S->yw.as<float4>(), Yds_out, out_memspace));      // (nothing has been peeled yet) exactly the fp32 video the session searches
    CK(hipStreamSynchronize(ctx->st()));                     // (Qpre is the caller's pageable memory; the tables of `c` go with this frame)
    return 0;
}

// cnmfe_peel_open_residual_ds: the session of the second pass on dsData(Yres) of the PATCH (@Sources2D/initComponents_residual_parallel.m:171-177,232 ->
// greedyROI_endoscope.m:46-61), Yres = Ysig - A(patch, ind) C(ind, :).  The caller has made sure that P->ysig holds the residual itself (residual_materialize).
// A_ds is formed here in float64 (ds_fold_csc), C_ds on the device (k_trace_bin_mean: a bound C never comes down), and k_ds_video_res writes the down-sampled
// difference straight into Yw: no full-resolution Yres exists.  The residual carries its own mean: no ymean, no k_ds_mean.
int peel_open_residual_ds_run(cnmfe_ctx *ctx, Patch *P, int ssub, int tsub, int32_t Ksel, const int64_t *A_colptr, const int32_t *A_rowidx, const float *A_val,
                              const float *C, int c_order, const float *psf, int32_t psf_n, float sig, float *Cn_out, float *PNR_out, float *Sn_out,
                              float *Yds_out, int out_memspace) {
    PeelSession *S = P->peel;
    const int64_t n = P->T, nq_in = (n + 3) / 4;
    DsCall c;
    DsTaps tr, tc;
    RET(ds_plan(ctx, P->nr, P->nc, P->d, ssub, tsub, n, c, &tr, &tc));
    S->n = c.Ts; S->nq = c.nq; S->M = 0; S->d = c.ds; S->nr = c.d1s; S->nc = c.d2s; S->residual = true;
    const size_t vid = (size_t)c.nq * (size_t)c.ds * sizeof(float4);
    if (S->hy.ensure(vid) != 0 || S->yw.ensure(vid) != 0) {
        (void)hipGetLastError();
        return fail(CNMFE_ENOMEM, "down-sampled residual peel session: no room for the filtered video and the working copy, 2 x %zu bytes (16 x ceil(Ts / 4) x d1s d2s = 16 x %lld x %lld)",
                    vid, (long long)c.nq, (long long)c.ds);
    }
    RET(S->sn.ensure((size_t)c.ds * sizeof(double)));
    RET(S->ci.ensure(peel_al((size_t)c.Ts * sizeof(double)) * 2));
    // (buffers of this call: released when it returns, behind the stream's last wait)
    DevBuf dC, dCds, dRow, dCol, dVal;
    const bool has_ac = Ksel > 0 && A_colptr[Ksel] > 0;
    if (has_ac) {
        DsCSR fold;
        if (!ds_fold_csc(P->nr, P->nc, tr, tc, Ksel, A_colptr, A_rowidx, A_val, fold))
            return fail(CNMFE_EUNSUPPORTED, "down-sampled residual peel session: the low-resolution footprints hold 2^31 entries or more");
        int64_t ldc = 4;
        RET(upload_traces(ctx, dC, C, Ksel, n, c_order, &ldc));
        RET(dCds.ensure((size_t)Ksel * (size_t)c.Ts * sizeof(double)));
        LAUNCH(ctx, "trace_bin_mean", k_trace_bin_mean, dim3((unsigned)((c.Ts + 255) / 256), (unsigned)Ksel), dim3(256), 0, dC.as<float>(), ldc, tsub, (int)c.Ts, dCds.as<double>());
        RET(to_dev(ctx, dRow, fold.rowptr)); RET(to_dev(ctx, dCol, fold.col)); RET(to_dev(ctx, dVal, fold.val));
    }
    DS_LAUNCH_NT(ctx, "ds_video_res", k_ds_video_res, std::max(c.g.ntr, c.g.ntc), dim3((unsigned)((c.ds + 255) / 256), (unsigned)c.nq), P->ysig.as<float4>(), (int)nq_in, c.g,
                 tsub, (int)c.Ts, has_ac ? dRow.as<int>() : (const int *)nullptr, dCol.as<int>(), dVal.as<double>(), dCds.as<double>(), S->yw.as<float4>());
    RET(seed_images_run(ctx, SeedSrc{S->yw.as<float4>(), c.ds, c.d1s, c.d2s}, psf, psf_n, c.Ts, nullptr, 0, sig, Cn_out, PNR_out, S));
    if (Sn_out) {
        std::vector<double> sn((size_t)c.ds);
        CK(hipMemcpyAsync(sn.data(), S->sn.p, (size_t)c.ds * sizeof(double), hipMemcpyDeviceToHost, ctx->st()));
        CK(hipStreamSynchronize(ctx->st()));
        for (int64_t i = 0; i < c.ds; ++i) Sn_out[i] = (float)sn[(size_t)i];
    }
    if (Yds_out) RET(ds_export(ctx, c, S->yw.as<float4>(), Yds_out, out_memspace));      // (nothing has been peeled yet) exactly the fp32 video the session searches
    CK(hipStreamSynchronize(ctx->st()));                     // (the tables of `c` and the buffers of this frame are read until here)
    return 0;
}

}  // namespace cnmfe
