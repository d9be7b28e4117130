// (f) closing calls: the six panels of show_demixed_video   @Sources2D/show_demixed_video.m:70-81,94-127 (raw, background, raw - background, denoised A C, residual,
// pseudo-coloured demixed), of the displayed frames t_j = frame0 + j stride of one patch.
// Included by resid.hip below bg_reconstruct_run: the background of a frame is k_bg_out's expression on the same operands (Yc, Ysig, the per-pixel constant kappa of
// k_rss_const), so `bg` has the bits cnmfe_reconstruct_background writes; with bg_ssub > 1 it is read from the slab cnmfe_reconstruct_background_ssub just wrote.
//   k_demix_panels    one thread per (patch pixel, displayed frame); lanes run along pixels, so the quads yc4[q d_b + p] and ysig4[q d + p] coalesce (frame t is component
//                     t % 4 of quad t / 4); the pixel's CSR row of A and the wave's few trace values come from L2 (k_peel_yres' pattern); 64-bit offsets throughout.
// Every (pixel, frame, panel) is written by exactly one thread with a plain store, every sum runs over the pixel's stored neurons in ascending column order: equal
// inputs give equal bits, whatever the lanes.  A block pixel outside the patch is never addressed: the grid covers the patch's d pixels only.
#pragma once

namespace cnmfe {

// MATLAB's uint16(): round half away from zero, saturate to [0, 65535], NaN -> 0
__device__ __forceinline__ unsigned short demix_u16(double v) {
    if (!(v == v)) return 0;
    const double r = round(v);
    return (unsigned short)(r <= 0.0 ? 0.0 : (r >= 65535.0 ? 65535.0 : r));
}

// SLAB: the background of frame t lies at bgslab[(t - slab0) d + m] (bg_ssub > 1); else it is rebuilt from Ysig and kappa as k_bg_out rebuilds it.
// arow / acol / aval: the CSR rows of the patch's A (acol = position in the call's neuron list), trow[k] = row of neuron k in the trace matrix CC (stride ldc),
// col: Ksel x 3.  out.mixed: three planes of nframes x d.
template <bool SLAB>
__global__ void __launch_bounds__(256) k_demix_panels(const float4 *__restrict__ yc4, int64_t d_b, int nr, int nr_b, int roff, int coff, const float4 *__restrict__ ysig4,
                                                      int64_t d, const float *__restrict__ ymean_f, const float *__restrict__ kappa, const float *__restrict__ bgslab,
                                                      int64_t slab0, const int *__restrict__ arow, const int *__restrict__ acol, const float *__restrict__ aval,
                                                      const int *__restrict__ trow, const float *__restrict__ CC, int64_t ldc, const float *__restrict__ col,
                                                      double mix_scale, int64_t frame0, int64_t stride, int64_t nframes, DemixOut out) {
    const int64_t m = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (m >= d) return;
    const int64_t j = blockIdx.y;
    const int64_t q = (int64_t)((int)(m / nr) + coff) * nr_b + (int)(m % nr) + roff;
    const int64_t t = frame0 + j * stride, c = t >> 2; const int u = (int)(t & 3);
    const float ym = ymean_f[q];
    const float y = reinterpret_cast<const float *>(yc4 + c * d_b + q)[u];
    const float raw = y + ym;
    float bg;
    if constexpr (SLAB) bg = bgslab[(t - slab0) * d + m];
    else {
        const float cst = ym - kappa[m];
        const float s = reinterpret_cast<const float *>(ysig4 + c * d + m)[u];
        bg = y - s + cst;                                     // (k_bg_out's expression, in its order)
    }
    double acc = 0.0, mx0 = 0.0, mx1 = 0.0, mx2 = 0.0;
    if (arow)
        for (int e = arow[m]; e < arow[m + 1]; ++e) {
            const int k = acol[e];
            const double a = (double)aval[e], cv = (double)CC[(int64_t)trow[k] * ldc + t];
            acc = fma(a, cv, acc);
            mx0 = fma(a, (double)col[3 * k] * cv, mx0);       // (fp32 x fp32 is exact in fp64: col(k, m) CC(k, t) as the reference forms it first)
            mx1 = fma(a, (double)col[3 * k + 1] * cv, mx1);
            mx2 = fma(a, (double)col[3 * k + 2] * cv, mx2);
        }
    const int64_t o = j * d + m;
    if (out.raw) out.raw[o] = raw;
    if (out.bg) out.bg[o] = bg;
    if (out.signal) out.signal[o] = raw - bg;
    if (out.denoised) out.denoised[o] = (float)acc;
    if (out.residual) out.residual[o] = (float)((double)raw - (double)bg - acc);
    if (out.mixed) {
        const int64_t plane = nframes * d;
        out.mixed[o] = demix_u16(mix_scale * mx0);
        out.mixed[plane + o] = demix_u16(mix_scale * mx1);
        out.mixed[2 * plane + o] = demix_u16(mix_scale * mx2);
    }
}

// background_model = 'svd': the same panels on bg = (float)(b0(m) + sum_i b(m, i) f(i, t)), an fp64 fma chain over ascending i rounded once -- the patch's fp64
// factors (bg_svd.hpp), no Ysig and no kappa, so no residual is asked for.  A sibling of k_demix_panels rather than a third flavour: the two instantiations above keep
// their code.  The workgroup shares t (blockIdx.y): f(i, t) is one address for all lanes; b's columns b[i d + m] coalesce along pixels.
__global__ void __launch_bounds__(256) k_demix_panels_lowrank(const float4 *__restrict__ yc4, int64_t d_b, int nr, int nr_b, int roff, int coff, int64_t d,
                                                              const float *__restrict__ ymean_f, const double *__restrict__ b0, const double *__restrict__ b,
                                                              const double *__restrict__ f, int nb, int64_t T, const int *__restrict__ arow, const int *__restrict__ acol,
                                                              const float *__restrict__ aval, const int *__restrict__ trow, const float *__restrict__ CC, int64_t ldc,
                                                              const float *__restrict__ col, double mix_scale, int64_t frame0, int64_t stride, int64_t nframes, DemixOut out) {
    const int64_t m = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (m >= d) return;
    const int64_t j = blockIdx.y;
    const int64_t q = (int64_t)((int)(m / nr) + coff) * nr_b + (int)(m % nr) + roff;
    const int64_t t = frame0 + j * stride, c = t >> 2; const int u = (int)(t & 3);
    const float y = reinterpret_cast<const float *>(yc4 + c * d_b + q)[u];
    const float raw = y + ymean_f[q];
    double bf = b0[m];
    for (int i = 0; i < nb; ++i) bf = fma(b[(int64_t)i * d + m], f[(int64_t)i * T + t], bf);
    const float bg = (float)bf;
    double acc = 0.0, mx0 = 0.0, mx1 = 0.0, mx2 = 0.0;
    if (arow)
        for (int e = arow[m]; e < arow[m + 1]; ++e) {
            const int k = acol[e];
            const double a = (double)aval[e], cv = (double)CC[(int64_t)trow[k] * ldc + t];
            acc = fma(a, cv, acc);
            mx0 = fma(a, (double)col[3 * k] * cv, mx0);
            mx1 = fma(a, (double)col[3 * k + 1] * cv, mx1);
            mx2 = fma(a, (double)col[3 * k + 2] * cv, mx2);
        }
    const int64_t o = j * d + m;
    if (out.raw) out.raw[o] = raw;
    if (out.bg) out.bg[o] = bg;
    if (out.signal) out.signal[o] = raw - bg;
    if (out.denoised) out.denoised[o] = (float)acc;
    if (out.residual) out.residual[o] = (float)((double)raw - (double)bg - acc);
    if (out.mixed) {
        const int64_t plane = nframes * d;
        out.mixed[o] = demix_u16(mix_scale * mx0);
        out.mixed[plane + o] = demix_u16(mix_scale * mx1);
        out.mixed[2 * plane + o] = demix_u16(mix_scale * mx2);
    }
}

// ---- host side ----------------------------------------------------------------------------------------------

// the call's A (CSR over the patch pixels), trace rows and colours on the active lane (every index was checked by the caller)
int demix_stage(cnmfe_ctx *ctx, Patch *P, int32_t Ksel, const int64_t *cp, const int32_t *ri, const float *va, const int32_t *trow, const float *col) {
    if (Ksel <= 0) return 0;
    HostCSR csr;
    csc_to_csr(P->d, Ksel, cp, ri, va, csr);
    RET(to_dev(ctx, ctx->dmx[0], csr.rowptr)); RET(to_dev(ctx, ctx->dmx[1], csr.col)); RET(to_dev(ctx, ctx->dmx[2], csr.val));
    RET(to_dev(ctx, ctx->dmx[3], trow, (size_t)Ksel)); RET(to_dev(ctx, ctx->dmx[4], col, (size_t)Ksel * 3));
    return 0;
}

// kappa of the patch for (b0_block, b0_new) in tmp[12], as bg_reconstruct_run leaves it (bg_ssub = 1; the residual is materialised first)
int demix_kappa(cnmfe_ctx *ctx, Patch *P, const float *b0_block, const float *b0_new) {
    RET(residual_materialize(ctx, P));
    return bg_kappa(ctx, P, b0_block, b0_new);
}

// displayed frames [j0, j0 + nj) of the call's nframes; slab: the background of the contiguous frames from slab0 on (bg_ssub > 1), nullptr: from Ysig and tmp[12].
// The outputs are device pointers to whole panels (nframes x d).
int demix_launch(cnmfe_ctx *ctx, Patch *P, int32_t Ksel, const float *dCC, int64_t ldc, double mix_scale, int64_t frame0, int64_t stride, int64_t nframes, int64_t j0,
                 int64_t nj, const float *slab, int64_t slab0, const DemixOut &out) {
    if (nj <= 0) return 0;
    DemixOut o = out;
    const int64_t off = j0 * P->d;
    if (o.raw) o.raw += off; if (o.bg) o.bg += off; if (o.signal) o.signal += off; if (o.denoised) o.denoised += off; if (o.residual) o.residual += off;
    if (o.mixed) o.mixed += off;                               // (the planes stay nframes x d apart: the kernel is told the call's nframes)
    const int *arow = Ksel > 0 ? ctx->dmx[0].as<int>() : (const int *)nullptr;
    const dim3 grid((unsigned)((P->d + 255) / 256), (unsigned)nj);
    const int64_t f0 = frame0 + j0 * stride;
    if (slab)
        LAUNCH(ctx, "demix_panels", k_demix_panels<true>, grid, dim3(256), 0, P->Yc4.as<float4>(), P->d_b, P->nr, P->nr_b, P->roff, P->coff, (const float4 *)nullptr, P->d,
               P->ymean_f.as<float>(), (const float *)nullptr, slab, slab0, arow, ctx->dmx[1].as<int>(), ctx->dmx[2].as<float>(), ctx->dmx[3].as<int>(), dCC, ldc,
               ctx->dmx[4].as<float>(), mix_scale, f0, stride, nframes, o);
    else
        LAUNCH(ctx, "demix_panels", k_demix_panels<false>, grid, dim3(256), 0, P->Yc4.as<float4>(), P->d_b, P->nr, P->nr_b, P->roff, P->coff, P->ysig.as<float4>(), P->d,
               P->ymean_f.as<float>(), ctx->tmp[12].as<float>(), (const float *)nullptr, int64_t(0), arow, ctx->dmx[1].as<int>(), ctx->dmx[2].as<float>(),
               ctx->dmx[3].as<int>(), dCC, ldc, ctx->dmx[4].as<float>(), mix_scale, f0, stride, nframes, o);
    return 0;
}

// all nframes displayed frames of the call under the patch's low-rank factors (the caller has checked P->svd_nb >= 0 and the frames)
int demix_launch_lowrank(cnmfe_ctx *ctx, Patch *P, int32_t Ksel, const float *dCC, int64_t ldc, double mix_scale, int64_t frame0, int64_t stride, int64_t nframes,
                         const DemixOut &out) {
    if (nframes <= 0) return 0;
    const int *arow = Ksel > 0 ? ctx->dmx[0].as<int>() : (const int *)nullptr;
    const dim3 grid((unsigned)((P->d + 255) / 256), (unsigned)nframes);
    LAUNCH(ctx, "demix_panels_lowrank", k_demix_panels_lowrank, grid, dim3(256), 0, P->Yc4.as<float4>(), P->d_b, P->nr, P->nr_b, P->roff, P->coff, P->d,
           P->ymean_f.as<float>(), P->svd_b0.as<double>(), P->svd_b.as<double>(), P->svd_f.as<double>(), P->svd_nb, P->T, arow, ctx->dmx[1].as<int>(),
           ctx->dmx[2].as<float>(), ctx->dmx[3].as<int>(), dCC, ldc, ctx->dmx[4].as<float>(), mix_scale, frame0, stride, nframes, out);
    return 0;
}

}  // namespace cnmfe
