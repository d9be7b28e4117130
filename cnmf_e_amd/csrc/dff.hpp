// (i) dF/F: [C_df, C_raw_df, Df] = extract_DF_F_endoscope(obj, Ybg)   @Sources2D/Sources2D.m:540-570, utilities/running_percentile.m:74-121
// Included by deconv.hip below merge.hpp (the baselines' exact order statistics are peel.hpp's 64-bit radix keys, the trace sources are merge.hpp's).  The background
// never exists as a whole: a patch's frames are reconstructed a chunk at a time into a lane's scratch (api.hip, cnmfe_df_add_background[_ssub]) and projected onto
// the footprints at once; what stays is the K x T fp64 accumulator of the context.
//   k_df_project      acc[ind[j], frame0 + t] += sum_i A(i, j) Ybg(i, t): fp32 x fp32 formed and summed in fp64, one wave per frame, plain read-add-write
//   k_df_scale        Yf = acc ./ sum(A.^2, 1)' in place (:545), and per row whether anything in it is not finite
//   k_df_base         Df(k) = median / Hazen percentile of row k (:549-553): one workgroup per trace, select_pair64 on the row in LDS or, long flavour, where it lies
//   k_df_base_win     Df(k, t) = medfilt1(., w, 'truncate') (:559) or running_percentile(., w, p) (:563): one thread per output sample, a 2-bit radix selection over
//                     its window of the row's 64-bit keys (LDS, or computed from the row in global memory: the long flavour)
//   k_df_divide       (float)((double)X / Df), row-wise or elementwise (:554-555, :567-568)
// Every reduction runs in a fixed order and every (row, frame) of the accumulator is written by one wave per call: equal inputs give equal bits, with any number of lanes
// (the projections of different lanes are chained by an event in call order: two patches may hold pixels of one neuron).
#pragma once

namespace cnmfe {

constexpr int DF_RUN = 64;            // frames per workgroup of k_df_project (16 per wave)
constexpr int DF_STAGE = 2048;        // stored pixels of one neuron kept in LDS (16 KB); a larger footprint is read from global memory every frame
constexpr int DF_WINDOW_MAX = 16384;  // include/cnmfe.h: the largest df_window served
constexpr size_t DF_LDS_MAX = 160 * 1024;
constexpr size_t DF_CHUNK_BYTES = size_t(256) << 20;      // the chunk scratch: at most the last-level cache, so the product reads what was just written

// One workgroup per (neuron j of the call, run of DF_RUN frames), one wave per frame at a time; the lanes stride over the neuron's stored pixels (ascending rows =
// down the image columns: the gather is mostly coalesced).  Butterfly reduction: the same order in every lane and every run.
__global__ void __launch_bounds__(256) k_df_project(const float *__restrict__ Y, int64_t d, int nframes, const int64_t *__restrict__ colptr, const int *__restrict__ rowidx,
                                                    const float *__restrict__ val, const int *__restrict__ ind, double *__restrict__ acc, int64_t ld, int64_t frame0) {
    extern __shared__ __attribute__((aligned(16))) unsigned char df_sm[];
    int *s_ri = reinterpret_cast<int *>(df_sm);
    float *s_va = reinterpret_cast<float *>(df_sm + (size_t)DF_STAGE * 4);
    const int j = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int64_t e0 = colptr[j];
    const int n = (int)(colptr[j + 1] - e0);
    if (n == 0) return;                                      // (an empty column adds nothing; uniform over the workgroup)
    const bool staged = n <= DF_STAGE;
    if (staged) {
        for (int e = tid; e < n; e += 256) { s_ri[e] = rowidx[e0 + e]; s_va[e] = val[e0 + e]; }
        __syncthreads();
    }
    const int *ri = staged ? s_ri : rowidx + e0;
    const float *va = staged ? s_va : val + e0;
    double *arow = acc + (int64_t)ind[j] * ld + frame0;
    const int t1 = min(nframes, ((int)blockIdx.y + 1) * DF_RUN);
    for (int t = (int)blockIdx.y * DF_RUN + wave; t < t1; t += 4) {
        const float *y = Y + (int64_t)t * d;
        double s = 0.0;
        for (int e = lane; e < n; e += 64) s += (double)va[e] * (double)y[ri[e]];
        for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o);
        if (lane == 0) arow[t] += s;
    }
}

// Yf(k, :) = acc(k, :) * inv[k] in place; bad[k] = 1 when the row then holds anything that is not finite (an empty footprint: 0 * Inf)
__global__ void __launch_bounds__(256) k_df_scale(double *__restrict__ acc, int64_t ld, int64_t T, const double *__restrict__ inv, int *__restrict__ bad) {
    double *row = acc + (int64_t)blockIdx.x * ld;
    const double s = inv[blockIdx.x];
    int b = 0;
    for (int64_t t = threadIdx.x; t < T; t += 256) { const double v = row[t] * s; row[t] = v; b |= !isfinite(v); }
    b = __syncthreads_or(b);
    if (threadIdx.x == 0) bad[blockIdx.x] = b;
}

__device__ __forceinline__ double df_nan() { return __longlong_as_double(0x7ff8000000000000ll); }

// Df(k) of the whole row: median(Yf, 2) when p == 50 (an even count: the mean of the two middle samples), else prctile(Yf, p, 2) = the Hazen rule (sorted sample i at
// 100 (i - 0.5) / n, linear in between, the minimum / maximum outside; the arithmetic of oracle.cnmfe_oracle.matlab_quantile).  LONG: the row is read where it lies.
template <bool LONG>
__global__ void __launch_bounds__(256) k_df_base(const double *__restrict__ Yf, int64_t ld, int T, double p, const int *__restrict__ bad, double *__restrict__ Df) {
    extern __shared__ __attribute__((aligned(16))) unsigned char df_sm[];
    const int k = blockIdx.x, tid = threadIdx.x;
    if (bad[k]) { if (tid == 0) Df[k] = df_nan(); return; }
    const double *row = Yf + (int64_t)k * ld;
    int *hist = reinterpret_cast<int *>(df_sm);              // 264 ints, then the row (16-byte aligned: 1072)
    const double *y = row;
    if constexpr (!LONG) {
        double *ys = reinterpret_cast<double *>(df_sm + 1072);
        for (int t = tid; t < T; t += 256) ys[t] = row[t];
        __syncthreads();
        y = ys;
    }
    int k0; double g = 0.0; bool med2 = false;
    if (p == 50.0) { k0 = (T - 1) / 2; med2 = !(T & 1); }
    else {
        const double r = (p / 100.0) * (double)T + 0.5;       // 1-based fractional rank
        if (r <= 1.0) k0 = 0;
        else if (r >= (double)T) k0 = T - 1;
        else { const double lo = floor(r); k0 = (int)lo - 1; g = r - lo; }
    }
    double vk, vk1;
    select_pair64(y, T, k0, hist, vk, vk1);
    if (tid == 0) Df[k] = med2 ? 0.5 * (vk + vk1) : (g == 0.0 ? vk : vk + g * (vk1 - vk));
}

// The two windowed baselines, one thread per output sample t.  mode 0 = medfilt1(Yf, w, [], 2, 'truncate'): window t - (w - 1) / 2 .. t + (w - 1) / 2 (odd w) or
// t - w / 2 .. t + w / 2 - 1 (even w), clipped to the trace, the median of what remains.  mode 1 = running_percentile (:76-78, :90-104): window
// t - (ceil(w / 2) - 1) .. t + floor(w / 2), the trace reflected at both ends with the edge sample repeated, pt = p w / 100 + 0.5.
// The order statistic kk (and its successor) of the window comes from a radix selection on the 64-bit keys, two bits per pass.
template <bool LONG>
__global__ void __launch_bounds__(256) k_df_base_win(const double *__restrict__ Yf, int64_t ld, int T, int w, double p, int mode, const int *__restrict__ bad,
                                                     double *__restrict__ Df) {
    extern __shared__ __attribute__((aligned(16))) unsigned char df_sm[];
    const int k = blockIdx.x, tid = threadIdx.x;
    const double *row = Yf + (int64_t)k * ld;
    double *out = Df + (int64_t)k * T;
    if (bad[k]) { for (int t = tid; t < T; t += 256) out[t] = df_nan(); return; }
    unsigned long long *keys = reinterpret_cast<unsigned long long *>(df_sm);
    if constexpr (!LONG) {
        for (int t = tid; t < T; t += 256) keys[t] = dkey(row[t]);
        __syncthreads();
    }
    auto key_at = [&](int j) -> unsigned long long {
        const int i = j < 0 ? -j - 1 : (j >= T ? 2 * T - 1 - j : j);
        if constexpr (LONG) return dkey(row[i]); else return keys[i];
    };
    // what mode 1 asks of every window alike
    int kk1 = 0; bool pair1 = false; double xf = 0.0;
    if (mode == 1) {
        const double pt = p * (double)w / 100.0 + 0.5;
        if (pt < 1.0) kk1 = 0;
        else if (pt > (double)w) kk1 = w - 1;
        else if (floor(pt) == pt) kk1 = (int)pt - 1;
        else {
            const double f = floor(pt), x0 = 100.0 * (f - 0.5) / (double)w, x1 = 100.0 * (f + 0.5) / (double)w;
            kk1 = (int)f - 1; pair1 = true; xf = (p - x0) / (x1 - x0);
        }
    }
    for (int t = tid; t < T; t += 256) {
        int a, b, kk; bool pair;
        if (mode == 0) {
            a = (w & 1) ? t - (w - 1) / 2 : t - w / 2;
            b = (w & 1) ? t + (w - 1) / 2 : t + w / 2 - 1;
            a = a < 0 ? 0 : a; b = b > T - 1 ? T - 1 : b;
            const int n = b - a + 1;
            kk = (n - 1) / 2; pair = !(n & 1);
        } else { a = t - ((w + 1) / 2 - 1); b = t + w / 2; kk = kk1; pair = pair1; }
        unsigned long long prefix = 0, known = 0;
        for (int shift = 62; shift >= 0; shift -= 2) {
            int c0 = 0, c1 = 0, c2 = 0;
            for (int j = a; j <= b; ++j) {
                const unsigned long long key = key_at(j);
                if ((key & known) == prefix) { const int dg = (int)((key >> shift) & 3); c0 += dg == 0; c1 += dg == 1; c2 += dg == 2; }
            }
            unsigned long long dg;
            if (kk < c0) dg = 0;
            else if (kk < c0 + c1) { kk -= c0; dg = 1; }
            else if (kk < c0 + c1 + c2) { kk -= c0 + c1; dg = 2; }
            else { kk -= c0 + c1 + c2; dg = 3; }
            prefix |= dg << shift; known |= 3ull << shift;
        }
        const double vk = dkey_inv(prefix);
        double r = vk;
        if (pair) {                                          // the successor: the same value while it repeats, else the smallest key above
            int ce = 0; unsigned long long mn = ~0ull;
            for (int j = a; j <= b; ++j) { const unsigned long long key = key_at(j); ce += key == prefix; if (key > prefix && key < mn) mn = key; }
            const double vk1 = (kk + 1 < ce || mn == ~0ull) ? vk : dkey_inv(mn);
            r = mode == 0 ? 0.5 * (vk + vk1) : vk + (vk1 - vk) * xf;
        }
        out[t] = r;
    }
}

// out(k, t) = (float)((double)X(k, t) / Df), Df per row (ldf = 0) or per sample (ldf = T); out is K x T, dense
__global__ void __launch_bounds__(256) k_df_divide(const float *__restrict__ X, int64_t ldc, const double *__restrict__ Df, int64_t ldf, int64_t T, float *__restrict__ out) {
    const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x, k = blockIdx.y;
    if (t >= T) return;
    const double den = ldf ? Df[k * ldf + t] : Df[k];
    out[k * T + t] = (float)((double)X[k * ldc + t] / den);
}

// ---- host side ----------------------------------------------------------------------------------------------

int df_begin_run(cnmfe_ctx *ctx, int32_t K, int64_t T) {
    const size_t bytes = (size_t)std::max<int64_t>(1, (int64_t)K * T) * 8;
    RET(ctx->df_acc.ensure(bytes));
    CK(hipMemsetAsync(ctx->df_acc.p, 0, bytes, ctx->st()));
    ctx->df_K = K; ctx->df_T = T; ctx->df_open = true; ctx->df_chain = false;
    return 0;
}

// the footprints and rows of one call, on the active lane (every index was checked by the caller)
int df_stage_a(cnmfe_ctx *ctx, int32_t Km, const int64_t *cp, const int32_t *ri, const float *va, const int32_t *ind) {
    RET(to_dev(ctx, ctx->dfl[1], cp, (size_t)Km + 1)); RET(to_dev(ctx, ctx->dfl[2], ri, (size_t)cp[Km])); RET(to_dev(ctx, ctx->dfl[3], va, (size_t)cp[Km]));
    RET(to_dev(ctx, ctx->dfl[4], ind, (size_t)Km));
    return 0;
}

// acc[ind, frame0 + (0 .. nframes)) += A' dY with the staged A; dY: d x nframes frame-major on the device.  With lanes the projections follow each other in call order.
int df_project_run(cnmfe_ctx *ctx, int32_t Km, int64_t d, int64_t frame0, int64_t nframes, const float *dY) {
    if (Km <= 0 || nframes <= 0) return 0;
    if (!ctx->lanes.empty()) {
        if (!ctx->ev_df) CK(hipEventCreateWithFlags(&ctx->ev_df, hipEventDisableTiming));
        if (ctx->df_chain) CK(hipStreamWaitEvent(ctx->st(), ctx->ev_df, 0));
    }
    LAUNCH(ctx, "df_project", k_df_project, dim3((unsigned)Km, (unsigned)((nframes + DF_RUN - 1) / DF_RUN)), dim3(256), (size_t)DF_STAGE * 8, dY, d, (int)nframes,
           ctx->dfl[1].as<int64_t>(), ctx->dfl[2].as<int>(), ctx->dfl[3].as<float>(), ctx->dfl[4].as<int>(), ctx->df_acc.as<double>(), ctx->df_T, frame0);
    if (!ctx->lanes.empty()) { CK(hipEventRecord(ctx->ev_df, ctx->st())); ctx->df_chain = true; }
    return 0;
}

int df_add_frames_run(cnmfe_ctx *ctx, int64_t d, int64_t frame0, int64_t nframes, const float *Ybg, int memspace, int32_t Km, const int64_t *cp, const int32_t *ri,
                      const float *va, const int32_t *ind) {
    RET(df_stage_a(ctx, Km, cp, ri, va, ind));
    const float *dY = Ybg;
    if (memspace != CNMFE_DEVICE) {
        RET(ctx->dfl[0].ensure((size_t)d * nframes * 4));
        CK(hipMemcpyAsync(ctx->dfl[0].p, Ybg, (size_t)d * nframes * 4, hipMemcpyHostToDevice, ctx->st()));
        dY = ctx->dfl[0].as<float>();
    }
    RET(df_project_run(ctx, Km, d, frame0, nframes, dY));
    CK(hipStreamSynchronize(ctx->st()));                     // (the caller's buffers are free again)
    return ctx_check_errflag(ctx);
}

// frames per chunk of a patch of d pixels: a multiple of 4, at most DF_CHUNK_BYTES of scratch and what one reconstruction call hands out
int df_chunk_frames(int64_t d, int64_t T, int64_t *nch) {
    int64_t n = (int64_t)(DF_CHUNK_BYTES / ((size_t)d * 4)) & ~int64_t(3);
    if (n < 4) return fail(CNMFE_EUNSUPPORTED, "a patch of %lld pixels does not fit four frames into the %zu MB chunk scratch", (long long)d, DF_CHUNK_BYTES >> 20);
    n = std::min<int64_t>(n, 65532);
    *nch = std::min<int64_t>(n, (T + 3) & ~int64_t(3));
    return 0;
}
float *df_chunk_buf(cnmfe_ctx *ctx, int64_t d, int64_t nch) { return ctx->dfl[0].ensure((size_t)d * nch * 4) == 0 ? ctx->dfl[0].as<float>() : nullptr; }

int df_fetch_run(cnmfe_ctx *ctx, double *out) {
    if (ctx->df_K > 0) CK(hipMemcpyAsync(out, ctx->df_acc.p, (size_t)ctx->df_K * ctx->df_T * 8, hipMemcpyDeviceToHost, ctx->st()));
    CK(hipStreamSynchronize(ctx->st()));
    return ctx_check_errflag(ctx);
}

int df_load_run(cnmfe_ctx *ctx, int32_t K, int64_t T, const double *Yf) {
    if (!ctx->df_open) RET(df_begin_run(ctx, K, T));
    if (K > 0) CK(hipMemcpyAsync(ctx->df_acc.p, Yf, (size_t)K * T * 8, hipMemcpyHostToDevice, ctx->st()));
    CK(hipStreamSynchronize(ctx->st()));
    return 0;
}

// a source the context must hold is asked for before anything of the accumulator changes (a host source cannot fail later)
int df_source_check(cnmfe_ctx *ctx, int32_t K, int64_t T, int src) {
    const float *dX;
    return (src == CNMFE_COLMAJOR || src == CNMFE_ROWMAJOR) ? 0 : merge_source(ctx, K, T, nullptr, src, &dX);
}

int df_finish_run(cnmfe_ctx *ctx, const double *inv_norm, double p, int64_t w, const float *C, int c_src, const float *C_raw, int raw_src, float *C_df_out,
                  float *C_raw_df_out, double *Df_out, double *Yf_out) {
    const int32_t K = ctx->df_K; const int64_t T = ctx->df_T;
    if (K == 0 || (!C_df_out && !C_raw_df_out && !Df_out && !Yf_out)) { ctx->df_open = false; return 0; }      // (nobody asks for anything: the accumulator is only closed)
    if (C_df_out) RET(df_source_check(ctx, K, T, c_src));
    if (C_raw_df_out) RET(df_source_check(ctx, K, T, raw_src));
    const bool win = w > 0;
    DevBuf &dInv = ctx->df_buf[0], &dBad = ctx->df_buf[1], &dDf = ctx->df_buf[2], &dOut = ctx->df_buf[3];
    RET(to_dev(ctx, dInv, inv_norm, (size_t)K));
    RET(dBad.ensure((size_t)K * 4)); RET(dDf.ensure((size_t)K * (win ? T : 1) * 8)); RET(dOut.ensure((size_t)K * T * 4));
    double *acc = ctx->df_acc.as<double>();
    LAUNCH(ctx, "df_scale", k_df_scale, dim3((unsigned)K), dim3(256), 0, acc, T, T, dInv.as<double>(), dBad.as<int>());
    // the flavour rule of seed.hpp / merge.hpp: the trace in LDS while it fits, where it lies beyond (or with option trace_long); equal bits where both run
    const size_t shmem = (win ? 0 : 1072) + (size_t)T * 8;
    const bool lng = shmem > DF_LDS_MAX || ctx->opt("trace_long", 0) != 0;
    if (!win) {
        if (lng) LAUNCH(ctx, "df_base", k_df_base<true>, dim3((unsigned)K), dim3(256), 1072, acc, T, (int)T, p, dBad.as<int>(), dDf.as<double>());
        else {
            if (shmem > 64 * 1024) CK(hipFuncSetAttribute((const void *)k_df_base<false>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)shmem));
            LAUNCH(ctx, "df_base", k_df_base<false>, dim3((unsigned)K), dim3(256), shmem, acc, T, (int)T, p, dBad.as<int>(), dDf.as<double>());
        }
    } else {
        const int mode = p == 50.0 ? 0 : 1;
        if (lng) LAUNCH(ctx, "df_base_win", k_df_base_win<true>, dim3((unsigned)K), dim3(256), 0, acc, T, (int)T, (int)w, p, mode, dBad.as<int>(), dDf.as<double>());
        else {
            if (shmem > 64 * 1024) CK(hipFuncSetAttribute((const void *)k_df_base_win<false>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)shmem));
            LAUNCH(ctx, "df_base_win", k_df_base_win<false>, dim3((unsigned)K), dim3(256), shmem, acc, T, (int)T, (int)w, p, mode, dBad.as<int>(), dDf.as<double>());
        }
    }
    const int64_t ldc = (T + 3) & ~int64_t(3);
    const dim3 grid((unsigned)((T + 255) / 256), (unsigned)K);
    const float *srcs[2] = {C, C_raw}; const int kinds[2] = {c_src, raw_src}; float *outs[2] = {C_df_out, C_raw_df_out};
    for (int m = 0; m < 2; ++m) {                            // (one after the other: two host sources share the upload buffer)
        if (!outs[m]) continue;
        const float *dX;
        RET(merge_source(ctx, K, T, srcs[m], kinds[m], &dX));
        LAUNCH(ctx, "df_divide", k_df_divide, grid, dim3(256), 0, dX, ldc, dDf.as<double>(), win ? T : int64_t(0), T, dOut.as<float>());
        CK(hipMemcpyAsync(outs[m], dOut.p, (size_t)K * T * 4, hipMemcpyDeviceToHost, ctx->st()));
    }
    if (Df_out) CK(hipMemcpyAsync(Df_out, dDf.p, (size_t)K * (win ? T : 1) * 8, hipMemcpyDeviceToHost, ctx->st()));
    if (Yf_out) CK(hipMemcpyAsync(Yf_out, acc, (size_t)K * T * 8, hipMemcpyDeviceToHost, ctx->st()));
    CK(hipStreamSynchronize(ctx->st()));
    ctx->df_open = false;
    return ctx_check_errflag(ctx);
}

}  // namespace cnmfe
