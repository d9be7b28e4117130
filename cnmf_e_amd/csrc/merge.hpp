// (h) merging: what the merge / tag methods of the demo loop read and write of the K x T trace matrices, where they lie.
//   @Sources2D/merge_high_corr.m:50-85,172-196,236   merge_neurons_dist_corr.m:58-86,180-201,243   merge_close_neighbors.m:49-83,174-195,237
//   @Sources2D/Sources2D.m:744-759 (remove_false_positives), :1683-1715 (tag_neurons_parallel)
// Included by deconv.hip below get_sn / block_sum / k_deconv's launcher (the merged row is deconvolved by the same kernel, the tags' and the S-less branch's noise
// levels are the same Welch estimator).  The K x K criteria, the connected components and the n x n alternation of a group stay on the host in float64
// (sources2d.py, hostops.py); the device does what is K x T:
//   k_trace_moments + k_trace_corr   corr(X') / X X' in fp64 on the fp64 matrix pipe (the pattern of k_trace_gram, win_proj_i8.hpp; the mean is subtracted in fp64
//                                    inside the kernel, per operand, so nothing of the fp32-centred copy's seven digits enters)
//   k_trace_diff_spikes              S_ = diff(C_raw) with a zero last column, entries below 2 GetSn(S_) zeroed (merge_high_corr.m:57-66)
//   k_trace_tags                     max(C), std(C_raw - C), GetSn(C_raw), |{S(2:end) > 0}| per trace in one pass (Sources2D.m:1700-1709)
//                                    (both: the trace in LDS beside the Welch transform up to 20416 frames; k_trace_diff_spikes_long / k_trace_tags_long beyond, up
//                                    to WELCH_TMAX = 147456 -- the difference trace in its output row, C_raw's row read in place, no scratch but the tables' slots)
//   k_merge_rows + k_merge_compact   ci = w' C_raw(IDs, :) in fp64, rounded once; the rows that stay, gathered into new matrices that are swapped in
//   k_trace_energy (+ _fin)          sum(X.^2, 2) in fp64, one pass: the weights of batch mode's footprint average (update_spatial_batch.m:29)
// Every reduction runs in a fixed order: equal inputs give equal bits (on every rank of a sharded run).
#pragma once

namespace cnmfe {

typedef double mg_double4 __attribute__((ext_vector_type(4)));

// mean and centred sum of squares of every row, fp64, two passes, fixed order (thread-strided partial sums, then block_sum's tree)
__global__ void __launch_bounds__(256) k_trace_moments(const float *__restrict__ X, int64_t ldc, int64_t T, double *__restrict__ mean, double *__restrict__ css) {
    __shared__ double red[4];
    const float *row = X + (int64_t)blockIdx.x * ldc;
    double s = 0;
    for (int64_t t = threadIdx.x; t < T; t += 256) s += (double)row[t];
    const double m = block_sum(s, red) / (double)T;
    double q = 0;
    for (int64_t t = threadIdx.x; t < T; t += 256) { const double d = (double)row[t] - m; q += d * d; }
    q = block_sum(q, red);
    if (threadIdx.x == 0) { mean[blockIdx.x] = m; css[blockIdx.x] = q; }
}

// G[k * K + l] = sum_t (X_k(t) - m_k)(X_l(t) - m_l) / sqrt(css_k css_l)   (raw: sum_t X_k(t) X_l(t)), fp64: one workgroup per 16 x 16 tile of the upper triangle,
// mirrored on store; its sixteen waves take a sixteenth of the frames each and are summed in wave order.  Frames behind T contribute exact zeros whatever the
// padding holds.  A row without variance has css = 0 exactly (the mean of T equal fp32 values is that value in fp64): 0 / 0 = NaN in its row and column.
constexpr int MG_W = 16;
__global__ void __launch_bounds__(64 * MG_W) k_trace_corr(const float *__restrict__ X, int64_t ldc, int64_t T, int K, const double *__restrict__ mean,
                                                          const double *__restrict__ css, int raw, double *__restrict__ G) {
    __shared__ double red[MG_W - 1][64][4];
    const int nt = (K + 15) >> 4;
    int ti = 0, rem = blockIdx.x;                          // blockIdx.x enumerates (ti <= tj)
    while (rem >= nt - ti) { rem -= nt - ti; ++ti; }
    const int tj = ti + rem;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, fi = lane & 15, kq = lane >> 4;
    const int ka = min(ti * 16 + fi, K - 1), kb = min(tj * 16 + fi, K - 1);
    const float4 *ra = reinterpret_cast<const float4 *>(X + (int64_t)ka * ldc);
    const float4 *rb = reinterpret_cast<const float4 *>(X + (int64_t)kb * ldc);
    const double ma = raw ? 0.0 : mean[ka], mb = raw ? 0.0 : mean[kb];
    const int64_t nch = (T + 3) >> 2;                      // ldc = 4 nch: every chunk read lies inside the row
    const int64_t per = (((nch + MG_W - 1) / MG_W) + 3) & ~int64_t(3), c0 = wave * per, c1 = c0 + per < nch ? c0 + per : nch;
    mg_double4 acc = {0.0, 0.0, 0.0, 0.0};
    for (int64_t s = c0; s < c1; s += 16) {
        float4 a[4], b[4]; int nv[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int64_t c = s + 4 * u + kq;
            a[u] = make_float4(0.f, 0.f, 0.f, 0.f); b[u] = a[u]; nv[u] = 0;
            if (c < c1) { a[u] = ra[c]; b[u] = rb[c]; const int64_t left = T - 4 * c; nv[u] = left > 4 ? 4 : (int)left; }
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int n = nv[u];
            acc = __builtin_amdgcn_mfma_f64_16x16x4f64(n > 0 ? (double)a[u].x - ma : 0.0, n > 0 ? (double)b[u].x - mb : 0.0, acc, 0, 0, 0);
            acc = __builtin_amdgcn_mfma_f64_16x16x4f64(n > 1 ? (double)a[u].y - ma : 0.0, n > 1 ? (double)b[u].y - mb : 0.0, acc, 0, 0, 0);
            acc = __builtin_amdgcn_mfma_f64_16x16x4f64(n > 2 ? (double)a[u].z - ma : 0.0, n > 2 ? (double)b[u].z - mb : 0.0, acc, 0, 0, 0);
            acc = __builtin_amdgcn_mfma_f64_16x16x4f64(n > 3 ? (double)a[u].w - ma : 0.0, n > 3 ? (double)b[u].w - mb : 0.0, acc, 0, 0, 0);
        }
    }
    if (wave) {
#pragma unroll
        for (int r = 0; r < 4; ++r) red[wave - 1][lane][r] = acc[r];
    }
    __syncthreads();
    if (wave == 0) {
#pragma unroll
        for (int r = 0; r < 4; ++r) {                      // D layout (fp64 16x16): row = kq + 4 r, column = fi; the partial sums in wave order
            double v = acc[r];
#pragma unroll
            for (int w2 = 0; w2 < MG_W - 1; ++w2) v += red[w2][lane][r];
            const int k = ti * 16 + kq + 4 * r, l = tj * 16 + fi;
            if (k < K && l < K) {
                if (!raw) v = v / (sqrt(css[k]) * sqrt(css[l]));
                G[(int64_t)k * K + l] = v; G[(int64_t)l * K + k] = v;
            }
        }
    }
}

// merge_high_corr.m:59-65: one workgroup per trace, the difference trace in LDS for the Welch estimator
__global__ void __launch_bounds__(256) k_trace_diff_spikes(DeconvCfg c, const float *__restrict__ X, int64_t ldc, float *__restrict__ out, float *__restrict__ sn_out) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    __shared__ double red[4];
    const int tid = threadIdx.x, T = c.T, Tal = (T + 3) & ~3;
    const float *row = X + (int64_t)blockIdx.x * ldc;
    float *y = lds, *scr = lds + Tal;
    for (int t = tid; t < Tal; t += 256) y[t] = t < T - 1 ? row[t + 1] - row[t] : 0.f;       // S_(:, end + 1) = 0
    __syncthreads();
    const double sn = get_sn(y, c, scr, red, false);
    float *o = out + (int64_t)blockIdx.x * ldc;
    for (int t = tid; t < (int)ldc; t += 256) o[t] = (t < T && !((double)y[t] < 2.0 * sn)) ? y[t] : 0.f;
    if (tid == 0 && sn_out) sn_out[blockIdx.x] = (float)sn;
}

// Sources2D.m:1700-1709, per trace: out[4 k ..] = max(C), std(C_raw - C, 0) (fp64, N - 1), GetSn(C_raw), |{S(2:end) > 0}| (-1 without an S)
__global__ void __launch_bounds__(256) k_trace_tags(DeconvCfg c, const float *__restrict__ Cm, const float *__restrict__ Craw, const float *__restrict__ S, int64_t ldc,
                                                    double *__restrict__ out) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    __shared__ double red[4];
    __shared__ float mred[4];
    const int tid = threadIdx.x, T = c.T, Tal = (T + 3) & ~3;
    const int64_t off = (int64_t)blockIdx.x * ldc;
    float *y = lds, *scr = lds + Tal;
    float mx = -INFINITY; double s = 0, cnt = 0;
    for (int t = tid; t < Tal; t += 256) {
        const float r = t < T ? Craw[off + t] : 0.f;
        y[t] = r;
        if (t < T) { const float cv = Cm[off + t]; mx = fmaxf(mx, cv); s += (double)r - (double)cv; if (S && t >= 1 && S[off + t] > 0.f) cnt += 1; }
    }
    for (int o = 32; o > 0; o >>= 1) mx = fmaxf(mx, __shfl_xor(mx, o));
    if ((tid & 63) == 0) mred[tid >> 6] = mx;
    const double m = block_sum(s, red) / (double)T;            // (its barriers publish y and mred)
    cnt = block_sum(cnt, red);
    double q = 0;
    for (int t = tid; t < T; t += 256) { const double d = ((double)y[t] - (double)Cm[off + t]) - m; q += d * d; }
    q = block_sum(q, red);
    const double sn = get_sn(y, c, scr, red, false);
    if (tid == 0) {
        double *o = out + 4 * (int64_t)blockIdx.x;
        o[0] = (double)fmaxf(fmaxf(mred[0], mred[1]), fmaxf(mred[2], mred[3]));
        o[1] = sqrt(q / (double)(T > 1 ? T - 1 : 1)); o[2] = sn; o[3] = S ? cnt : -1.0;
    }
}

// The long flavours (welch_cfg, deconv.hip): a workgroup walks the traces blockIdx.x, blockIdx.x + gridDim.x, ...; no trace lives in LDS, which holds the
// transform alone.  The difference trace is written to its output row first, read from there by get_sn and thresholded in place; the tags read C_raw's row where
// it lies.  Same threads, strides and sums as the LDS flavours: equal bits where both run.
template <bool SPLIT>
__global__ void __launch_bounds__(256) k_trace_diff_spikes_long(DeconvCfg c, float *__restrict__ tabs, const float *__restrict__ X, int64_t ldc, int K,
                                                                float *__restrict__ out, float *__restrict__ sn_out) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    __shared__ double red[4];
    const int tid = threadIdx.x, T = c.T, Tal = (T + 3) & ~3;
    for (int k = blockIdx.x; k < K; k += gridDim.x) {
        const float *row = X + (int64_t)k * ldc;
        float *y = out + (int64_t)k * ldc;                   // (ldc = ceil4(T): the row is the LDS flavour's copy, padding included)
        for (int t = tid; t < Tal; t += 256) y[t] = t < T - 1 ? row[t + 1] - row[t] : 0.f;
        __threadfence_block();
        __syncthreads();
        const double sn = get_sn_long<SPLIT>(y, c, lds, red, tabs);
        for (int t = tid; t < (int)ldc; t += 256) { const float v = y[t]; y[t] = (t < T && !((double)v < 2.0 * sn)) ? v : 0.f; }
        if (tid == 0 && sn_out) sn_out[k] = (float)sn;
        __syncthreads();
    }
}

template <bool SPLIT>
__global__ void __launch_bounds__(256) k_trace_tags_long(DeconvCfg c, float *__restrict__ tabs, const float *__restrict__ Cm, const float *__restrict__ Craw,
                                                         const float *__restrict__ S, int64_t ldc, int K, double *__restrict__ out) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    __shared__ double red[4];
    __shared__ float mred[4];
    const int tid = threadIdx.x, T = c.T;
    for (int k = blockIdx.x; k < K; k += gridDim.x) {
        const int64_t off = (int64_t)k * ldc;
        const float *y = Craw + off;
        float mx = -INFINITY; double s = 0, cnt = 0;
        for (int t = tid; t < T; t += 256) {
            const float r = y[t], cv = Cm[off + t];
            mx = fmaxf(mx, cv); s += (double)r - (double)cv; if (S && t >= 1 && S[off + t] > 0.f) cnt += 1;
        }
        for (int o = 32; o > 0; o >>= 1) mx = fmaxf(mx, __shfl_xor(mx, o));
        if ((tid & 63) == 0) mred[tid >> 6] = mx;
        const double m = block_sum(s, red) / (double)T;            // (its barriers publish mred)
        cnt = block_sum(cnt, red);
        double q = 0;
        for (int t = tid; t < T; t += 256) { const double d = ((double)y[t] - (double)Cm[off + t]) - m; q += d * d; }
        q = block_sum(q, red);
        const double sn = get_sn_long<SPLIT>(y, c, lds, red, tabs);
        if (tid == 0) {
            double *o = out + 4 * (int64_t)k;
            o[0] = (double)fmaxf(fmaxf(mred[0], mred[1]), fmaxf(mred[2], mred[3]));
            o[1] = sqrt(q / (double)(T > 1 ? T - 1 : 1)); o[2] = sn; o[3] = S ? cnt : -1.0;
        }
        __syncthreads();                                     // (the next trace rewrites mred)
    }
}

// ci = w' C_raw(IDs, :) of group g: fp64 sum in the group's order, rounded to fp32 once; written twice (mci stays, mraw is what k_deconv reads and rewrites)
__global__ void __launch_bounds__(256) k_merge_rows(const float *__restrict__ Craw, int64_t ldc, int64_t T, const int *__restrict__ gptr, const int *__restrict__ gidx,
                                                    const double *__restrict__ w, float *__restrict__ mci, float *__restrict__ mraw) {
    const int g = blockIdx.x, j0 = gptr[g], j1 = gptr[g + 1];
    for (int64_t t = threadIdx.x; t < ldc; t += 256) {
        double a = 0;
        if (t < T) for (int j = j0; j < j1; ++j) a += w[j] * (double)Craw[(int64_t)gidx[j] * ldc + t];
        const float v = (float)a;
        mci[(int64_t)g * ldc + t] = v; mraw[(int64_t)g * ldc + t] = v;
    }
}

// row j of the new matrices = row keep[j] of the old ones, or the merged group's row where mrg[j] >= 0; blockIdx.y = which matrix (C, C_raw, S)
struct MergeMats { const float4 *old_[3]; const float4 *mrg_[3]; float4 *new_[3]; };
__global__ void __launch_bounds__(256) k_merge_compact(MergeMats mm, int64_t ldc4, const int *__restrict__ keep, const int *__restrict__ mrg,
                                                       const float *__restrict__ pars_old, const float *__restrict__ sn_old, const float *__restrict__ pars_m,
                                                       const float *__restrict__ sn_m, float *__restrict__ pars_new, float *__restrict__ sn_new) {
    const int j = blockIdx.x, y = blockIdx.y, g = mrg[j];
    const float4 *s = g >= 0 ? mm.mrg_[y] + (int64_t)g * ldc4 : mm.old_[y] + (int64_t)keep[j] * ldc4;
    float4 *d = mm.new_[y] + (int64_t)j * ldc4;
    for (int64_t c = threadIdx.x; c < ldc4; c += 256) d[c] = s[c];
    if (y == 0 && threadIdx.x == 0) { pars_new[j] = g >= 0 ? pars_m[g] : pars_old[keep[j]]; sn_new[j] = g >= 0 ? sn_m[g] : sn_old[keep[j]]; }
}

// out[k] = sum_t X(k, t)^2 in fp64 (update_spatial_batch.m:29: cc = sum(neuron_k.C.^2, 2)).  One pass over the padded pitch with float4 loads, as k_merge_compact
// reads it: workgroup (s, k) takes segment s of row k, TE_SEG4 float4 chunks = 4 per thread.  A thread sums its squares in chunk order (an fp32 square is exact in
// fp64), block_sum adds the threads -- the wave's butterfly, then the four waves through LDS -- and k_trace_energy_fin the segments of a row, lane-strided in
// segment order and through the same butterfly.  No atomics, nothing depends on the launch's timing: equal inputs give equal bits.  Frames behind T
// contribute exact zeros whatever the padding holds.
constexpr int TE_SEG4 = 1024;
__global__ void __launch_bounds__(256) k_trace_energy(const float4 *__restrict__ X, int64_t ldc4, int64_t T, int nseg, double *__restrict__ part) {
    __shared__ double red[4];
    const int k = blockIdx.y, sg = blockIdx.x;
    const float4 *row = X + (int64_t)k * ldc4;
    const int64_t c0 = (int64_t)sg * TE_SEG4 + threadIdx.x;
    float4 v[4]; int nv[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
        const int64_t c = c0 + 256 * u;
        v[u] = make_float4(0.f, 0.f, 0.f, 0.f); nv[u] = 0;
        if (c < ldc4) { v[u] = row[c]; const int64_t left = T - 4 * c; nv[u] = left > 4 ? 4 : (int)left; }      // (ldc4 = ceil(T / 4): left >= 1)
    }
    double a = 0;
#pragma unroll
    for (int u = 0; u < 4; ++u) {
        const double x = (double)v[u].x, y = (double)v[u].y, z = (double)v[u].z, w = (double)v[u].w;
        if (nv[u] > 0) a += x * x;
        if (nv[u] > 1) a += y * y;
        if (nv[u] > 2) a += z * z;
        if (nv[u] > 3) a += w * w;
    }
    a = block_sum(a, red);
    if (threadIdx.x == 0) part[(int64_t)k * nseg + sg] = a;
}
__global__ void __launch_bounds__(64) k_trace_energy_fin(const double *__restrict__ part, int nseg, double *__restrict__ out) {
    const double *p = part + (int64_t)blockIdx.x * nseg;
    double a = 0;
    for (int s = threadIdx.x; s < nseg; s += 64) a += p[s];
    for (int o = 32; o > 0; o >>= 1) a += __shfl_xor(a, o);
    if (threadIdx.x == 0) out[blockIdx.x] = a;
}

// orderROIs' per-trace statistics (Sources2D.m:599-637) and the max(CC, [], 2) of show_demixed_video.m:37, one workgroup per trace, fp64: out[7 k ..] = mean(C),
// var(C, 0), var(C_raw - C, 0), max(C), ||C_raw||_2, ||C_raw||_1, max(C_raw).  Two passes (the means first), thread-strided partial sums and block_sum's tree: a
// fixed order.  T is a loop bound: nothing of the trace lives in LDS.
__global__ void __launch_bounds__(256) k_trace_order_stats(const float *__restrict__ Cm, const float *__restrict__ Craw, int64_t ldc, int64_t T, double *__restrict__ out) {
    __shared__ double red[4];
    __shared__ float mred[8];
    const int tid = threadIdx.x;
    const float *c = Cm + (int64_t)blockIdx.x * ldc, *r = Craw + (int64_t)blockIdx.x * ldc;
    float mc = -INFINITY, mr = -INFINITY;
    double sc = 0, sd = 0, s2 = 0, s1 = 0;
    for (int64_t t = tid; t < T; t += 256) {
        const float cv = c[t], rv = r[t];
        mc = fmaxf(mc, cv); mr = fmaxf(mr, rv);
        sc += (double)cv; sd += (double)rv - (double)cv; s2 += (double)rv * (double)rv; s1 += fabs((double)rv);
    }
    for (int o = 32; o > 0; o >>= 1) { mc = fmaxf(mc, __shfl_xor(mc, o)); mr = fmaxf(mr, __shfl_xor(mr, o)); }
    if ((tid & 63) == 0) { mred[tid >> 6] = mc; mred[4 + (tid >> 6)] = mr; }
    const double mean_c = block_sum(sc, red) / (double)T;      // (its barriers publish mred)
    const double mean_d = block_sum(sd, red) / (double)T;
    s2 = block_sum(s2, red); s1 = block_sum(s1, red);
    double qc = 0, qd = 0;
    for (int64_t t = tid; t < T; t += 256) {
        const double cv = (double)c[t], a = cv - mean_c, b = ((double)r[t] - cv) - mean_d;
        qc += a * a; qd += b * b;
    }
    qc = block_sum(qc, red); qd = block_sum(qd, red);
    if (tid == 0) {
        double *o = out + 7 * (int64_t)blockIdx.x;
        const double n1 = (double)(T > 1 ? T - 1 : 1);
        o[0] = mean_c; o[1] = qc / n1; o[2] = qd / n1;
        o[3] = (double)fmaxf(fmaxf(mred[0], mred[1]), fmaxf(mred[2], mred[3]));
        o[4] = sqrt(s2); o[5] = s1;
        o[6] = (double)fmaxf(fmaxf(mred[4], mred[5]), fmaxf(mred[6], mred[7]));
    }
}

// ---- host side ----------------------------------------------------------------------------------------------

// (welch_cfg / WelchPlan, the one Welch set-up of these kernels and of seed.hpp / peel.hpp, sits in deconv.hip beside sn_pixels_launch, whose tier rule it follows)

static bool residents_valid(const cnmfe_ctx *ctx) { return ctx->bound_valid && ctx->residents_gen == ctx->bound_gen; }

// the K x ldc device matrix a (X, src) argument names; host matrices go through mrg[0] and count as an upload
static int merge_source(cnmfe_ctx *ctx, int32_t K, int64_t T, const float *X, int src, const float **dX) {
    if (src == CNMFE_COLMAJOR || src == CNMFE_ROWMAJOR) {
        int64_t l2;
        RET(upload_traces(ctx, ctx->mrg[0], X, K, T, src, &l2));
        ++ctx->merge_uploads;
        *dX = ctx->mrg[0].as<float>();
        return 0;
    }
    if (src == CNMFE_BOUND) {
        if (!ctx->bound_valid || ctx->bound_K != K || ctx->bound_T != T) return fail(CNMFE_ESTATE, "no bound trace matrix of %d x %lld (cnmfe_traces_bind)", K, (long long)T);
        *dX = ctx->bound.as<float>();
        return 0;
    }
    if (src == CNMFE_RES_CRAW || src == CNMFE_RES_S) {
        if (!residents_valid(ctx) || ctx->bound_K != K || ctx->bound_T != T || (src == CNMFE_RES_S && !ctx->res_has_s))
            return fail(CNMFE_ESTATE, "the context holds no %s of %d x %lld beside its bound matrix (cnmfe_deconv_temporal_bound, cnmfe_traces_load)", src == CNMFE_RES_S ? "S" : "C_raw", K, (long long)T);
        *dX = (src == CNMFE_RES_S ? ctx->dcv_s : ctx->dcv_c).as<float>();
        return 0;
    }
    if (src == CNMFE_RES_DIFF) {
        if (ctx->diff_K != K || ctx->diff_T != T || ctx->diff_K <= 0) return fail(CNMFE_ESTATE, "no result of cnmfe_trace_diff_spikes of %d x %lld", K, (long long)T);
        *dX = ctx->mrg[1].as<float>();
        return 0;
    }
    return fail(CNMFE_EINVAL, "bad trace source %d", src);
}

int trace_corr_run(cnmfe_ctx *ctx, int32_t K, int64_t T, const float *X, int src, int raw, double *out) {
    const int64_t ldc = (T + 3) & ~int64_t(3);
    const float *dX;
    RET(merge_source(ctx, K, T, X, src, &dX));
    DevBuf &dMean = ctx->mrg[2], &dCss = ctx->mrg[3], &dG = ctx->mrg[4];
    RET(dMean.ensure((size_t)K * 8)); RET(dCss.ensure((size_t)K * 8)); RET(dG.ensure((size_t)K * K * 8));
    if (!raw) LAUNCH(ctx, "trace_moments", k_trace_moments, dim3((unsigned)K), dim3(256), 0, dX, ldc, T, dMean.as<double>(), dCss.as<double>());
    const int nt = (K + 15) >> 4;
    LAUNCH(ctx, "trace_corr", k_trace_corr, dim3((unsigned)(nt * (nt + 1) / 2)), dim3(64 * MG_W), 0, dX, ldc, T, (int)K, dMean.as<double>(), dCss.as<double>(), raw ? 1 : 0, dG.as<double>());
    CK(hipMemcpyAsync(out, dG.p, (size_t)K * K * 8, hipMemcpyDeviceToHost, ctx->st()));
    CK(hipStreamSynchronize(ctx->st()));
    return ctx_check_errflag(ctx);
}

// cnmfe_trace_energy: the source where it lies (a host matrix through mrg[0], counted as an upload), the partial sums in mrg[2], the K results in mrg[3]
int trace_energy_run(cnmfe_ctx *ctx, int32_t K, int64_t T, const float *X, int src, double *out) {
    const int64_t ldc = (T + 3) & ~int64_t(3), ldc4 = ldc >> 2;
    const int64_t nseg = (ldc4 + TE_SEG4 - 1) / TE_SEG4;
    if (nseg > 65535 || K > 65535) return fail(CNMFE_EINVAL, "cnmfe_trace_energy: %d x %lld is beyond one launch (65535 rows, %lld frames)", K, (long long)T, (long long)65535 * TE_SEG4 * 4);
    const float *dX;
    RET(merge_source(ctx, K, T, X, src, &dX));
    DevBuf &dPart = ctx->mrg[2], &dOut = ctx->mrg[3];
    RET(dPart.ensure((size_t)K * nseg * 8)); RET(dOut.ensure((size_t)K * 8));
    LAUNCH(ctx, "trace_energy", k_trace_energy, dim3((unsigned)nseg, (unsigned)K), dim3(256), 0, reinterpret_cast<const float4 *>(dX), ldc4, T, (int)nseg, dPart.as<double>());
    LAUNCH(ctx, "trace_energy_fin", k_trace_energy_fin, dim3((unsigned)K), dim3(64), 0, (const double *)dPart.as<double>(), (int)nseg, dOut.as<double>());
    CK(hipMemcpyAsync(out, dOut.p, (size_t)K * 8, hipMemcpyDeviceToHost, ctx->st()));
    CK(hipStreamSynchronize(ctx->st()));
    return ctx_check_errflag(ctx);
}

// cnmfe_traces_grow: K_new - K zero rows under the bound matrix and, while they belong to it, under the residents; zero entries behind kernel_pars and sn.  Every
// matrix is rebuilt in a buffer of cnmfe_merge_apply (mrg[12..16]) -- the zero rows by a memset, the old rows by one device-to-device copy -- and swapped in, as
// that call swaps its compacted matrices in: the old allocation stays alive for a download that still reads it.  Nothing crosses PCIe.
int traces_grow_run(cnmfe_ctx *ctx, int32_t K_new) {
    const int32_t K = ctx->bound_K; const int64_t T = ctx->bound_T, ldc = (T + 3) & ~int64_t(3);
    const bool res = residents_valid(ctx);
    if (ctx->copy_pending) { CK(hipStreamWaitEvent(ctx->st(), ctx->ev_copy_done, 0)); ctx->copy_pending = false; }   // the last downloads still read bound / dcv_*
    const size_t ob = (size_t)K * ldc * 4, nb = (size_t)K_new * ldc * 4;
    DevBuf *mats[3] = {&ctx->bound, &ctx->dcv_c, &ctx->dcv_s}, *vecs[2] = {&ctx->dcv_pars, &ctx->dcv_sn};
    const int nm = res ? 3 : 1, nv = res ? 2 : 0;
    // every check and every allocation first: a failure leaves the context as it was
    for (int i = 0; i < nm; ++i)
        if (mats[i]->cap < ob) return fail(CNMFE_ESTATE, "cnmfe_traces_grow: matrix %d of the context holds fewer than %d x %lld floats", i, K, (long long)ldc);
    for (int i = 0; i < nv; ++i)
        if (vecs[i]->cap < (size_t)K * 4) return fail(CNMFE_ESTATE, "cnmfe_traces_grow: vector %d of the context holds fewer than %d floats", i, K);
    for (int i = 0; i < nm; ++i) RET(ctx->mrg[12 + i].ensure(nb));
    for (int i = 0; i < nv; ++i) RET(ctx->mrg[15 + i].ensure((size_t)K_new * 4));
    // the copies are queued into the side buffers, which nobody reads; only when all of them are queued do the buffers change places
    for (int i = 0; i < nm; ++i) {
        DevBuf &n = ctx->mrg[12 + i];
        CK(hipMemcpyAsync(n.p, mats[i]->p, ob, hipMemcpyDeviceToDevice, ctx->st()));
        CK(hipMemsetAsync((char *)n.p + ob, 0, nb - ob, ctx->st()));
    }
    for (int i = 0; i < nv; ++i) {
        DevBuf &n = ctx->mrg[15 + i];
        CK(hipMemcpyAsync(n.p, vecs[i]->p, (size_t)K * 4, hipMemcpyDeviceToDevice, ctx->st()));
        CK(hipMemsetAsync((char *)n.p + (size_t)K * 4, 0, (size_t)(K_new - K) * 4, ctx->st()));
    }
    for (int i = 0; i < nm; ++i) mats[i]->swap(ctx->mrg[12 + i]);
    for (int i = 0; i < nv; ++i) vecs[i]->swap(ctx->mrg[15 + i]);
    ++ctx->bound_gen;                                        // (tables derived from the bound matrix' rows were sized for K of them)
    if (res) ctx->residents_gen = ctx->bound_gen;
    ctx->bound_K = K_new;
    return 0;
}

int trace_diff_spikes_run(cnmfe_ctx *ctx, int32_t K, int64_t T, const float *X, int src, float *sn_out, float *S_out) {
    const int64_t ldc = (T + 3) & ~int64_t(3);
    if (src == CNMFE_RES_DIFF) return fail(CNMFE_EINVAL, "cnmfe_trace_diff_spikes cannot read its own result");
    WelchPlan w;
    RET(welch_cfg(ctx, T, w));
    const float *dX;
    RET(merge_source(ctx, K, T, X, src, &dX));
    ctx->diff_K = 0;
    DevBuf &dOut = ctx->mrg[1], &dSn = ctx->mrg[5];
    RET(dOut.ensure((size_t)K * ldc * 4)); RET(dSn.ensure((size_t)K * 4));
    if (w.lng) {
        const unsigned nwg = w.nwg(K);
        float *tabs;
        RET(welch_tabs(ctx, w, nwg, &tabs));
        WELCH_LAUNCH_LONG(ctx, "trace_diff_spikes", k_trace_diff_spikes_long, w, nwg, tabs, dX, ldc, (int)K, dOut.as<float>(), dSn.as<float>());
    } else {
        if (w.shmem > 64 * 1024) CK(hipFuncSetAttribute((const void *)k_trace_diff_spikes, hipFuncAttributeMaxDynamicSharedMemorySize, (int)w.shmem));
        LAUNCH(ctx, "trace_diff_spikes", k_trace_diff_spikes, dim3((unsigned)K), dim3(256), w.shmem, w.c, dX, ldc, dOut.as<float>(), dSn.as<float>());
    }
    ctx->diff_K = K; ctx->diff_T = T;
    if (sn_out) CK(hipMemcpyAsync(sn_out, dSn.p, (size_t)K * 4, hipMemcpyDeviceToHost, ctx->st()));
    if (S_out) CK(hipMemcpy2DAsync(S_out, T * 4, dOut.p, ldc * 4, T * 4, K, hipMemcpyDeviceToHost, ctx->st()));
    CK(hipStreamSynchronize(ctx->st()));
    return ctx_check_errflag(ctx);
}

int trace_tags_run(cnmfe_ctx *ctx, int32_t K, double *out) {
    if (!residents_valid(ctx) || ctx->bound_K != K) return fail(CNMFE_ESTATE, "the context holds no C, C_raw of %d traces (cnmfe_deconv_temporal_bound, cnmfe_traces_load)", K);
    const int64_t T = ctx->bound_T, ldc = (T + 3) & ~int64_t(3);
    WelchPlan w;
    RET(welch_cfg(ctx, T, w));
    DevBuf &dOut = ctx->mrg[4];
    RET(dOut.ensure((size_t)K * 4 * 8));
    const float *dS = ctx->res_has_s ? ctx->dcv_s.as<float>() : (const float *)nullptr;
    if (w.lng) {
        const unsigned nwg = w.nwg(K);
        float *tabs;
        RET(welch_tabs(ctx, w, nwg, &tabs));
        WELCH_LAUNCH_LONG(ctx, "trace_tags", k_trace_tags_long, w, nwg, tabs, (const float *)ctx->bound.as<float>(), (const float *)ctx->dcv_c.as<float>(), dS, ldc, (int)K, dOut.as<double>());
    } else {
        if (w.shmem > 64 * 1024) CK(hipFuncSetAttribute((const void *)k_trace_tags, hipFuncAttributeMaxDynamicSharedMemorySize, (int)w.shmem));
        LAUNCH(ctx, "trace_tags", k_trace_tags, dim3((unsigned)K), dim3(256), w.shmem, w.c, ctx->bound.as<float>(), ctx->dcv_c.as<float>(), dS, ldc, dOut.as<double>());
    }
    CK(hipMemcpyAsync(out, dOut.p, (size_t)K * 4 * 8, hipMemcpyDeviceToHost, ctx->st()));
    CK(hipStreamSynchronize(ctx->st()));
    return ctx_check_errflag(ctx);
}

int trace_source_dev(cnmfe_ctx *ctx, int32_t K, int64_t T, const float *X, int src, const float **dX) { return merge_source(ctx, K, T, X, src, dX); }

int trace_order_stats_run(cnmfe_ctx *ctx, int32_t K, double *out) {
    if (!residents_valid(ctx) || ctx->bound_K != K) return fail(CNMFE_ESTATE, "the context holds no C, C_raw of %d traces (cnmfe_deconv_temporal_bound, cnmfe_traces_load)", K);
    const int64_t T = ctx->bound_T, ldc = (T + 3) & ~int64_t(3);
    DevBuf &dOut = ctx->mrg[4];
    RET(dOut.ensure((size_t)K * 7 * 8));
    LAUNCH(ctx, "trace_order_stats", k_trace_order_stats, dim3((unsigned)K), dim3(256), 0, (const float *)ctx->bound.as<float>(), (const float *)ctx->dcv_c.as<float>(), ldc, T,
           dOut.as<double>());
    CK(hipMemcpyAsync(out, dOut.p, (size_t)K * 7 * 8, hipMemcpyDeviceToHost, ctx->st()));
    CK(hipStreamSynchronize(ctx->st()));
    return ctx_check_errflag(ctx);
}

// cnmfe_traces_load: C becomes the bound matrix, C_raw / S / kernel_pars the context's residents (what cnmfe_deconv_temporal_bound leaves), from the host
int traces_load_run(cnmfe_ctx *ctx, int32_t K, int64_t T, const float *C, const float *C_raw, const float *S, const float *pars, int c_order) {
    if (ctx->copy_pending) { CK(hipStreamWaitEvent(ctx->st(), ctx->ev_copy_done, 0)); ctx->copy_pending = false; }
    int64_t ldc;
    ctx->bound_valid = false; ++ctx->bound_gen;
    RET(upload_traces(ctx, ctx->bound, C, K, T, c_order, &ldc)); ++ctx->merge_uploads;
    RET(upload_traces(ctx, ctx->dcv_c, C_raw ? C_raw : C, K, T, c_order, &ldc)); ++ctx->merge_uploads;
    RET(ctx->dcv_s.ensure((size_t)K * ldc * 4));
    if (S) { RET(upload_traces(ctx, ctx->dcv_s, S, K, T, c_order, &ldc)); ++ctx->merge_uploads; }
    else CK(hipMemsetAsync(ctx->dcv_s.p, 0, (size_t)K * ldc * 4, ctx->st()));
    RET(ctx->dcv_pars.ensure((size_t)K * 4)); RET(ctx->dcv_sn.ensure((size_t)K * 4));
    CK(hipMemsetAsync(ctx->dcv_pars.p, 0, (size_t)K * 4, ctx->st())); CK(hipMemsetAsync(ctx->dcv_sn.p, 0, (size_t)K * 4, ctx->st()));
    if (pars) CK(hipMemcpyAsync(ctx->dcv_pars.p, pars, (size_t)K * 4, hipMemcpyHostToDevice, ctx->st()));
    CK(hipStreamSynchronize(ctx->st()));
    ctx->bound_K = K; ctx->bound_T = T; ctx->bound_order = c_order; ctx->bound_valid = true;
    ctx->residents_gen = ctx->bound_gen; ctx->res_has_s = S != nullptr;
    return 0;
}

int merge_apply_run(cnmfe_ctx *ctx, int32_t ng, const int32_t *gptr, const int32_t *gidx, const double *w, int32_t nkeep, const int32_t *keep,
                    const cnmfe_deconv_opts *opts, float *C_out, float *C_raw_out, float *S_out, float *pars_out, float *sn_out) {
    if (!residents_valid(ctx)) return fail(CNMFE_ESTATE, "the context holds no C, C_raw beside its bound matrix (cnmfe_deconv_temporal_bound, cnmfe_traces_load)");
    const int32_t K = ctx->bound_K; const int64_t T = ctx->bound_T, ldc = (T + 3) & ~int64_t(3);
    // everything the kernels index with is checked here: rows in [0, K), a group's kept member among the kept rows
    std::vector<int> mrg((size_t)std::max(nkeep, 1), -1), pos((size_t)K, -1);
    for (int32_t j = 0; j < nkeep; ++j) {
        if (keep[j] < 0 || keep[j] >= K || pos[keep[j]] >= 0) return fail(CNMFE_EINVAL, "keep[%d] = %d is out of range or repeated (%d traces)", j, keep[j], K);
        pos[keep[j]] = j;
    }
    if (ng > 0 && gptr[0] != 0) return fail(CNMFE_EINVAL, "group pointers must start at 0");
    for (int32_t g = 0; g < ng; ++g) {
        if (gptr[g + 1] <= gptr[g]) return fail(CNMFE_EINVAL, "group %d is empty", g);
        for (int32_t j = gptr[g]; j < gptr[g + 1]; ++j) if (gidx[j] < 0 || gidx[j] >= K) return fail(CNMFE_EINVAL, "group %d names trace %d of %d", g, gidx[j], K);
        const int p = pos[gidx[gptr[g]]];
        if (p < 0 || mrg[p] >= 0) return fail(CNMFE_EINVAL, "the first member of group %d (trace %d) must be kept, and by one group only", g, gidx[gptr[g]]);
        mrg[p] = g;
    }
    if (ctx->copy_pending) { CK(hipStreamWaitEvent(ctx->st(), ctx->ev_copy_done, 0)); ctx->copy_pending = false; }   // the last downloads still read bound / dcv_*
    DevBuf &mCi = ctx->mrg[6], &mRaw = ctx->mrg[7], &mC = ctx->mrg[8], &mS = ctx->mrg[9], &mPars = ctx->mrg[10], &mSn = ctx->mrg[11];
    DevBuf &nC = ctx->mrg[12], &nR = ctx->mrg[13], &nS = ctx->mrg[14], &nPars = ctx->mrg[15], &nSn = ctx->mrg[16];
    DevBuf &dGp = ctx->mrg[17], &dGi = ctx->mrg[18], &dW = ctx->mrg[19], &dKeep = ctx->mrg[20], &dMrg = ctx->mrg[21], &dList = ctx->mrg[22];
    const size_t gb = (size_t)std::max(ng, 1) * ldc * 4, kb = (size_t)std::max(nkeep, 1) * ldc * 4;
    if (ng > 0) {
        DeconvCfg c; size_t shmem;
        RET(deconv_setup(opts, T, 0, c, shmem));
        const int n = gptr[ng];
        RET(mCi.ensure(gb)); RET(mRaw.ensure(gb)); RET(mC.ensure(gb)); RET(mS.ensure(gb)); RET(mPars.ensure((size_t)ng * 4)); RET(mSn.ensure((size_t)ng * 4));
        RET(ctx->scr[20].ensure((size_t)ng * 4));
        RET(to_dev(ctx, dGp, gptr, (size_t)ng + 1)); RET(to_dev(ctx, dGi, gidx, (size_t)n)); RET(to_dev(ctx, dW, w, (size_t)n));
        LAUNCH(ctx, "merge_rows", k_merge_rows, dim3((unsigned)ng), dim3(256), 0, ctx->dcv_c.as<float>(), ldc, T, dGp.as<int>(), dGi.as<int>(), dW.as<double>(),
               mCi.as<float>(), mRaw.as<float>());
        CK(hipMemsetAsync(mC.p, 0, gb, ctx->st())); CK(hipMemsetAsync(mS.p, 0, gb, ctx->st()));
        CK(hipMemsetAsync(mPars.p, 0, (size_t)ng * 4, ctx->st())); CK(hipMemsetAsync(mSn.p, 0, (size_t)ng * 4, ctx->st()));   // a fresh time constant (deconv_options_0 carries none)
        std::vector<int> list((size_t)ng);
        for (int g = 0; g < ng; ++g) list[g] = g;
        RET(to_dev(ctx, dList, list.data(), list.size()));
        DeconvIO io;
        io.C = mC.as<float>(); io.Craw = mRaw.as<float>(); io.S = mS.as<float>(); io.ldc = ldc;
        io.U = nullptr; io.nptr = nullptr; io.nidx = nullptr; io.nval = nullptr; io.aa = nullptr;
        io.pars = mPars.as<float>(); io.sn_out = mSn.as<float>(); io.b_out = ctx->scr[20].as<float>();
        const int batch = 512;
        for (int g0 = 0; g0 < ng; g0 += batch) RET(deconv_launch(ctx, c, shmem, io, dList.as<int>() + g0, std::min(batch, ng - g0), ctx->dscr));
    }
    RET(nC.ensure(kb)); RET(nR.ensure(kb)); RET(nS.ensure(kb)); RET(nPars.ensure((size_t)std::max(nkeep, 1) * 4)); RET(nSn.ensure((size_t)std::max(nkeep, 1) * 4));
    if (nkeep > 0) {
        RET(to_dev(ctx, dKeep, keep, (size_t)nkeep)); RET(to_dev(ctx, dMrg, mrg.data(), (size_t)nkeep));
        MergeMats mm;
        mm.old_[0] = ctx->bound.as<float4>(); mm.old_[1] = ctx->dcv_c.as<float4>(); mm.old_[2] = ctx->dcv_s.as<float4>();
        mm.mrg_[0] = mC.as<float4>(); mm.mrg_[1] = mCi.as<float4>(); mm.mrg_[2] = mS.as<float4>();
        mm.new_[0] = nC.as<float4>(); mm.new_[1] = nR.as<float4>(); mm.new_[2] = nS.as<float4>();
        LAUNCH(ctx, "merge_compact", k_merge_compact, dim3((unsigned)nkeep, 3), dim3(256), 0, mm, ldc >> 2, dKeep.as<int>(), dMrg.as<int>(), ctx->dcv_pars.as<float>(),
               ctx->dcv_sn.as<float>(), mPars.as<float>(), mSn.as<float>(), nPars.as<float>(), nSn.as<float>());
    }
    ctx->bound.swap(nC); ctx->dcv_c.swap(nR); ctx->dcv_s.swap(nS); ctx->dcv_pars.swap(nPars); ctx->dcv_sn.swap(nSn);
    ++ctx->bound_gen;
    ctx->bound_K = nkeep; ctx->bound_order = CNMFE_ROWMAJOR; ctx->bound_valid = nkeep > 0;
    ctx->residents_gen = ctx->bound_gen; ctx->diff_K = 0;
    if (nkeep > 0) {
        const size_t rb = (size_t)T * 4, pb = (size_t)ldc * 4;
        if (C_out) CK(hipMemcpy2DAsync(C_out, rb, ctx->bound.p, pb, rb, nkeep, hipMemcpyDeviceToHost, ctx->st()));
        if (C_raw_out) CK(hipMemcpy2DAsync(C_raw_out, rb, ctx->dcv_c.p, pb, rb, nkeep, hipMemcpyDeviceToHost, ctx->st()));
        if (S_out) CK(hipMemcpy2DAsync(S_out, rb, ctx->dcv_s.p, pb, rb, nkeep, hipMemcpyDeviceToHost, ctx->st()));
        if (pars_out) CK(hipMemcpyAsync(pars_out, ctx->dcv_pars.p, (size_t)nkeep * 4, hipMemcpyDeviceToHost, ctx->st()));
        if (sn_out) CK(hipMemcpyAsync(sn_out, ctx->dcv_sn.p, (size_t)nkeep * 4, hipMemcpyDeviceToHost, ctx->st()));
    }
    CK(hipStreamSynchronize(ctx->st()));
    return ctx_check_errflag(ctx);
}

}  // namespace cnmfe
