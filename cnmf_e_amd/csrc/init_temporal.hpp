// (f) known footprints: the traces of given footprints and a given ring background on the resident video of a patch
//   @Sources2D/initTemporal.m:156-168 (ring branch) -> utilities/HALS_temporal.m:34-41 (the rough start), :48-68 / :70-104 (the sweeps)
//     AA = sum(A(patch, :).^2, 1);   Yt = (E - W) Y_block;   At = (E - W) A_block;
//     [~, C] = HALS_temporal(Yt, At, [], 10);   [~, C_raw] = HALS_temporal(Yt, At, C, 2, deconv_options)
// Included by factor.hip behind the temporal update (its level kernels, graph and schedule are reused as they are).
//
// Nothing of Yt is ever formed.  With the resident CENTRED video Yc:  U = At' Yt = B' Yc (+ a constant per row),  B = (E - W)' At, and likewise for the rough
// start's selection tmp_A of At.  Every row update of HALS_temporal ends in "minus its minimum" (:66) or in the baseline removal of the deconvolution branch
// (:78,88), so a constant added to a row of U or of the starting C changes no output of the PLAIN sweeps: there the constants are dropped.
// The deconvolution branch is the exception -- its GetSn (:79) sees the row before the baseline goes --: U stays the centred video's there too, and the kernel
// of those sweeps gets the raw video's constant per row (k_it_pixconst, k_it_rowconst) for the samples GetSn windows.
//   k_it_filter    At(m, k) = A(m, k) - sum_i W(m, i) A(m + o_i, k) on neuron k's BOX (the footprint's bounding box grown by the ring, clipped to the patch;
//                  outside it At(:, k) is exactly 0), in fp64 from the fp32 A and W, ring order.  A(q, k) is looked up by bisection in the sorted column.
//   k_it_colred    per neuron the sum of its At column (1 / sum: HALS_temporal.m:36) or of the squares of its tmp_A column (1 / .: :39-41, 0 -> 1); fixed tree
//   k_it_winner    per patch pixel the entries of tmpA = At ./ sum(At) that equal the row maximum over ALL K columns (:37: implicit zeros compete, NaN is ignored
//                  as MATLAB's max ignores it); tmp_A = At there, 0 elsewhere
//   k_it_gram      V = At' At on the pairs of neurons whose boxes meet, in fp64 (fixed tree per pair), rounded once to the fp32 the level kernels read
//   vproj_temporal both projections in ONE block-tiled pass over the video: the 2 K columns (At_k, tmp_A_k) go through the panel builder in fp64
//                  (k_vp_build_b<double>) and the fp64 / int8 projection of the temporal update.  A block that meets more than 64 columns: several passes
//                  (vproj_pass_plan), each its own launch set
//   k_it_split     U(k, :) and C0(k, :) = (tmp_A' Yc)(k, :) / sum(tmp_A(:, k).^2) out of the 2 K projected rows
// then iters_plain plain sweeps and iters_last more (plain, or the in-sweep AR(1) FOOPSI with fresh kernel parameters) on the SAME U and V, all on the dependency
// graph of temporal_run, built from the non-zeros of V.  No atomics; every reduction has a fixed order: two calls give the same bits.

struct ItBox { int r0, c0, h, w; };        // neuron k's box in PATCH coordinates (h = 0: At(:, k) = 0)

// value of the sorted sparse column [a0, a1) at block pixel q (0 when it is not stored)
__device__ __forceinline__ float it_find(const int *__restrict__ arow, const float *__restrict__ aval, int64_t a0, int64_t a1, int q) {
    int64_t lo = a0, hi = a1;
    while (lo < hi) { const int64_t mid = (lo + hi) >> 1; if (arow[mid] < q) lo = mid + 1; else hi = mid; }
    return (lo < a1 && arow[lo] == q) ? aval[lo] : 0.f;
}

__global__ void __launch_bounds__(256) k_it_filter(const int64_t *__restrict__ acp, const int *__restrict__ arow, const float *__restrict__ aval, const ItBox *__restrict__ box,
                                                   const int64_t *__restrict__ pos, int nr, int nr_b, int nc_b, int roff, int coff, int p, const int *__restrict__ dr,
                                                   const int *__restrict__ dc, const float *__restrict__ W, int64_t d, double *__restrict__ out) {
    const int k = blockIdx.x;
    const ItBox bx = box[k];
    const int n = bx.h * bx.w;
    const int64_t a0 = acp[k], a1 = acp[k + 1];
    double *o = out + pos[k];
    for (int e = blockIdx.y * 256 + threadIdx.x; e < n; e += 256 * gridDim.y) {
        const int r = bx.r0 + e % bx.h, c = bx.c0 + e / bx.h;
        const int64_t m = (int64_t)c * nr + r;
        const int rb = r + roff, cb = c + coff;
        double acc = 0.0;
        for (int i = 0; i < p; ++i) {
            const float w = W[(int64_t)i * d + m];
            const int rq = rb + dr[i], cq = cb + dc[i];
            if (w != 0.f && rq >= 0 && rq < nr_b && cq >= 0 && cq < nc_b) acc += (double)w * (double)it_find(arow, aval, a0, a1, cq * nr_b + rq);
        }
        o[e] = (double)it_find(arow, aval, a0, a1, cb * nr_b + rb) - acc;
    }
}

// SQ = false: out[k] = 1 / sum(x);  SQ = true: out[k] = 1 / sum(x.^2) with 0 -> 1.  x = column k: n = h w doubles at v + pos[k] + (SQ ? n : 0)
template <bool SQ>
__global__ void __launch_bounds__(256) k_it_colred(const double *__restrict__ v, const ItBox *__restrict__ box, const int64_t *__restrict__ pos, double *__restrict__ out) {
    __shared__ double red[256];
    const int k = blockIdx.x;
    const int n = box[k].h * box[k].w;
    const double *x = v + pos[k] + (SQ ? n : 0);
    double s = 0.0;
    for (int e = threadIdx.x; e < n; e += 256) s += SQ ? x[e] * x[e] : x[e];
    red[threadIdx.x] = s; __syncthreads();
    for (int o = 128; o > 0; o >>= 1) { if ((int)threadIdx.x < o) red[threadIdx.x] += red[threadIdx.x + o]; __syncthreads(); }
    if (threadIdx.x == 0) out[k] = SQ ? 1.0 / (red[0] == 0.0 ? 1.0 : red[0]) : 1.0 / red[0];
}

// one thread per patch pixel; rptr / rk / rpos: the pixel's neurons and where their At entries lie (tmp_A: hw[k] doubles further)
__global__ void __launch_bounds__(256) k_it_winner(const int *__restrict__ rptr, const int *__restrict__ rk, const int *__restrict__ rpos, const ItBox *__restrict__ box,
                                                   const double *__restrict__ inv, int K, int64_t d, double *__restrict__ v) {
    __shared__ int cnt[256];
    int c = 0;
    for (int k = threadIdx.x; k < K; k += 256) c += isfinite(inv[k]) ? 1 : 0;          // columns whose implicit zeros are zeros of tmpA (0 * Inf, 0 * NaN are NaN)
    cnt[threadIdx.x] = c; __syncthreads();
    for (int o = 128; o > 0; o >>= 1) { if ((int)threadIdx.x < o) cnt[threadIdx.x] += cnt[threadIdx.x + o]; __syncthreads(); }
    const int nfin = cnt[0];
    const int64_t m = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (m >= d) return;
    const int q0 = rptr[m], q1 = rptr[m + 1];
    if (q0 == q1) return;
    double mx = 0.0; bool any = false; int here = 0;
    for (int q = q0; q < q1; ++q) {
        const double iv = inv[rk[q]], t = v[rpos[q]] * iv;
        here += isfinite(iv) ? 1 : 0;
        if (t == t && (!any || t > mx)) { mx = t; any = true; }
    }
    if (nfin > here && (!any || 0.0 > mx)) { mx = 0.0; any = true; }
    for (int q = q0; q < q1; ++q) {
        const int k = rk[q];
        const double a = v[rpos[q]], t = a * inv[k];
        v[rpos[q] + box[k].h * box[k].w] = (any && t == mx) ? a : 0.0;
    }
}

// pairs[i] = (k, j, slot of (k, j), slot of (j, k)) in the neighbour lists; 64 threads per pair over the intersection of the two boxes
__global__ void __launch_bounds__(64) k_it_gram(const int4 *__restrict__ pairs, const ItBox *__restrict__ box, const int64_t *__restrict__ pos, const double *__restrict__ v,
                                                float *__restrict__ nval, double *__restrict__ aa64) {
    __shared__ double red[64];
    const int4 pr = pairs[blockIdx.x];
    const ItBox a = box[pr.x], b = box[pr.y];
    const int r0 = max(a.r0, b.r0), r1 = min(a.r0 + a.h, b.r0 + b.h), c0 = max(a.c0, b.c0), c1 = min(a.c0 + a.w, b.c0 + b.w);
    const int h = r1 - r0, n = (h > 0 && c1 > c0) ? h * (c1 - c0) : 0;
    const double *va = v + pos[pr.x], *vb = v + pos[pr.y];
    double s = 0.0;
    for (int e = threadIdx.x; e < n; e += 64) {
        const int r = r0 + e % h, c = c0 + e / h;
        s += va[(c - a.c0) * a.h + (r - a.r0)] * vb[(c - b.c0) * b.h + (r - b.r0)];
    }
    red[threadIdx.x] = s; __syncthreads();
    for (int o = 32; o > 0; o >>= 1) { if ((int)threadIdx.x < o) red[threadIdx.x] += red[threadIdx.x + o]; __syncthreads(); }
    if (threadIdx.x == 0) {
        nval[pr.z] = (float)red[0]; nval[pr.w] = (float)red[0];
        if (pr.x == pr.y) aa64[pr.x] = red[0];
    }
}

// U2 row 2 j = At_k' Yc, row 2 j + 1 = tmp_A_k' Yc  (j = where[k]):  U(k, :) = the first,  C0(k, :) = the second / sum(tmp_A(:, k).^2)
__global__ void __launch_bounds__(256) k_it_split(const float *__restrict__ U2, const int *__restrict__ where, const double *__restrict__ scale, int64_t ldc, int64_t T,
                                                  float *__restrict__ U, float *__restrict__ C) {
    const int k = blockIdx.y;
    const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (t >= ldc) return;
    const int64_t j = where[k];
    U[(int64_t)k * ldc + t] = t < T ? U2[(2 * j) * ldc + t] : 0.f;
    C[(int64_t)k * ldc + t] = t < T ? (float)((double)U2[(2 * j + 1) * ldc + t] * scale[k]) : 0.f;
}

// The deconvolution branch is NOT shift invariant: HALS_temporal.m:79 takes GetSn of ck_raw BEFORE the baseline goes (:88), and Welch's windowed periodogram
// leaks a row's offset into the band it averages.  The raw video's U is the centred video's plus the constant
//   cst(k) = At(:, k)' (E - W) Ymean,   g(m) = Ymean(m) - sum_i W(m, i) Ymean(m + o_i)
// so its row update (:62) lies off(k) = cst(k) / aa(k) above the centred one's -- thousands where the signal is tens, which an fp32 row cannot carry (2.4e-4 per
// sample, 1e-5 .. 4e-5 of the trace).  U stays centred; off(k), in fp64 (fixed tree), goes to k_deconv (DeconvIO::off), which adds it where GetSn reads the row
// and nowhere else: the median baseline, the quantile and every residual move with the row.
__global__ void __launch_bounds__(256) k_it_pixconst(const double *__restrict__ ymean, const float *__restrict__ W, int64_t d, int nr, int nr_b, int nc_b, int roff, int coff, int p,
                                                     const int *__restrict__ dr, const int *__restrict__ dc, double *__restrict__ g) {
    const int64_t m = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (m >= d) return;
    const int rb = (int)(m % nr) + roff, cb = (int)(m / nr) + coff;
    double acc = 0.0;
    for (int i = 0; i < p; ++i) {
        const float w = W[(int64_t)i * d + m];
        const int rq = rb + dr[i], cq = cb + dc[i];
        if (w != 0.f && rq >= 0 && rq < nr_b && cq >= 0 && cq < nc_b) acc += (double)w * ymean[(int64_t)cq * nr_b + rq];
    }
    g[m] = ymean[(int64_t)cb * nr_b + rb] - acc;
}
__global__ void __launch_bounds__(256) k_it_rowconst(const double *__restrict__ v, const ItBox *__restrict__ box, const int64_t *__restrict__ pos, const double *__restrict__ g, int nr,
                                                     const double *__restrict__ aa64, double *__restrict__ off) {
    __shared__ double red[256];
    const int k = blockIdx.x;
    const ItBox bx = box[k];
    const int n = bx.h * bx.w;
    const double *x = v + pos[k];
    double s = 0.0;
    for (int e = threadIdx.x; e < n; e += 256) s += x[e] * g[(int64_t)(bx.c0 + e / bx.h) * nr + bx.r0 + e % bx.h];
    red[threadIdx.x] = s; __syncthreads();
    for (int o = 128; o > 0; o >>= 1) { if ((int)threadIdx.x < o) red[threadIdx.x] += red[threadIdx.x + o]; __syncthreads(); }
    if (threadIdx.x == 0) off[k] = aa64[k] > 0.0 ? red[0] / aa64[k] : 0.0;          // (aa = 0: the row is never updated)
}

// levels of `iters` sweeps over the neurons `upd` with the neighbour lists nb (sorted, k itself included): flat list + offsets
static void it_schedule(cnmfe_ctx *ctx, int K, const std::vector<std::vector<int>> &nb, const std::vector<char> &upd, int iters, bool flag_last, bool *dag_on,
                        std::vector<std::vector<int>> &levels) {
    PairGraph g; g.lower.assign(K, {});
    for (int k = 0; k < K; ++k) for (int j : nb[k]) if (j < k) g.lower[k].push_back(j);
    *dag_on = ctx->opt("sweep_dag", 1) != 0 && iters > 1;
    if (*dag_on) { dag_schedule(K, g, upd, iters, flag_last, levels); return; }
    std::vector<int> lvl(K, 0);
    int nl = 0;
    for (int k = 0; k < K; ++k) {
        int l = 0;
        for (int a : g.lower[k]) if (upd[a]) l = std::max(l, lvl[a] + 1);
        lvl[k] = l;
        if (upd[k]) nl = std::max(nl, l + 1);
    }
    levels.assign(nl, {});
    for (int k = 0; k < K; ++k) if (upd[k]) levels[lvl[k]].push_back(k);
}

int init_temporal_run(cnmfe_ctx *ctx, Patch *P, int32_t K, const int64_t *A_colptr, const int32_t *A_rowidx, const float *A_val, int32_t iters_plain, int32_t iters_last,
                      const cnmfe_deconv_opts *dopts, float *C_out, float *C_raw_out, float *S_out, float *pars_out, float *sn_out, float *AA_out, int c_order, TemporalJob *job) {
    const int64_t T = P->T, d = P->d, nnzA = A_colptr[K];
    const int nr = P->nr, nc = P->nc, nr_b = P->nr_b, roff = P->roff, coff = P->coff;
    if (nnzA >= (int64_t(1) << 31)) return fail(CNMFE_EUNSUPPORTED, "nnz(A) too large");
    RET(ensure_ymean(ctx, P));
    HostTrace ht(ctx, "init_temporal");
    int Rr = 0;
    for (int i = 0; i < P->p; ++i) Rr = std::max(Rr, std::max(std::abs(P->dr[i]), std::abs(P->dc[i])));
    // ---- host: AA of the original footprints on the patch rows (:160), every neuron's box, the common pattern of At and tmp_A
    std::vector<float> AA((size_t)K, 0.f);
    std::vector<ItBox> box((size_t)K);
    std::vector<int64_t> pcolptr((size_t)K + 1, 0);
    for (int32_t k = 0; k < K; ++k) {
        int rmin = INT32_MAX, rmax = -1, cmin = INT32_MAX, cmax = -1;
        double s = 0.0;
        for (int64_t e = A_colptr[k]; e < A_colptr[k + 1]; ++e) {
            const int rb = A_rowidx[e] % nr_b, cb = A_rowidx[e] / nr_b;
            rmin = std::min(rmin, rb); rmax = std::max(rmax, rb); cmin = std::min(cmin, cb); cmax = std::max(cmax, cb);
            if (rb >= roff && rb < roff + nr && cb >= coff && cb < coff + nc) s += (double)A_val[e] * (double)A_val[e];
        }
        AA[k] = (float)s;
        ItBox b{0, 0, 0, 0};
        if (rmax >= 0) {
            const int r0 = std::max(0, rmin - Rr - roff), r1 = std::min(nr - 1, rmax + Rr - roff), c0 = std::max(0, cmin - Rr - coff), c1 = std::min(nc - 1, cmax + Rr - coff);
            if (r1 >= r0 && c1 >= c0) b = ItBox{r0, c0, r1 - r0 + 1, c1 - c0 + 1};
        }
        if (b.h == 0) b.w = 0;
        box[k] = b;
        pcolptr[k + 1] = pcolptr[k] + (int64_t)b.h * b.w;
    }
    const int64_t nnzt = pcolptr[K];
    if (nnzt >= (int64_t(1) << 29)) return fail(CNMFE_EUNSUPPORTED, "init_temporal: the ring-filtered footprints have %lld entries", (long long)nnzt);
    std::vector<int32_t> prow((size_t)std::max<int64_t>(1, nnzt));
    for (int32_t k = 0; k < K; ++k) {
        int64_t e = pcolptr[k];
        for (int j = 0; j < box[k].w; ++j) for (int i = 0; i < box[k].h; ++i) prow[e++] = (box[k].c0 + j) * nr + box[k].r0 + i;
    }
    // ---- the passes of the projection and the 2 K-column matrix (At_k, tmp_A_k) in pass order
    std::vector<int> pass_of;
    const int npass = vproj_pass_plan(P, K, pcolptr.data(), prow.data(), 2, pass_of);
    if (npass <= 0) return fail(CNMFE_EUNSUPPORTED, "init_temporal: ring radius %d is beyond the projection's panel window", P->radius);
    std::vector<int> order((size_t)K), where((size_t)K), pass_end((size_t)npass, 0);
    for (int k = 0; k < K; ++k) order[k] = k;
    std::stable_sort(order.begin(), order.end(), [&](int a, int b) { return pass_of[a] < pass_of[b]; });
    std::vector<int64_t> colptr2((size_t)2 * K + 1, 0), pos((size_t)K);
    std::vector<int32_t> erow2((size_t)std::max<int64_t>(1, 2 * nnzt));
    for (int j = 0; j < K; ++j) {
        const int k = order[j];
        const int64_t n = pcolptr[k + 1] - pcolptr[k];
        where[k] = j; pos[k] = colptr2[2 * j]; pass_end[pass_of[k]] = j + 1;
        colptr2[2 * j + 1] = colptr2[2 * j] + n; colptr2[2 * j + 2] = colptr2[2 * j + 1] + n;
        for (int rep = 0; rep < 2; ++rep) if (n) memcpy(&erow2[colptr2[2 * j + rep]], &prow[pcolptr[k]], (size_t)n * sizeof(int32_t));
    }
    for (int p = 1; p < npass; ++p) pass_end[p] = std::max(pass_end[p], pass_end[p - 1]);
    // per patch pixel its neurons and where their At entries lie
    HostCSR csr; csc_to_csr(d, K, pcolptr.data(), prow.data(), nullptr, csr);
    std::vector<int> rpos((size_t)std::max<int64_t>(1, nnzt));
    for (int64_t q = 0; q < nnzt; ++q) rpos[q] = (int)(pos[csr.col[q]] + (csr.src[q] - pcolptr[csr.col[q]]));
    // neighbour lists: the neurons whose boxes meet (k itself included); the pairs k <= j and their two slots
    std::vector<std::vector<int>> nb((size_t)K);
    {
        std::vector<int> byc((size_t)K);
        for (int k = 0; k < K; ++k) byc[k] = k;
        std::sort(byc.begin(), byc.end(), [&](int a, int b) { return box[a].c0 != box[b].c0 ? box[a].c0 < box[b].c0 : a < b; });
        for (int ia = 0; ia < K; ++ia) {
            const int a = byc[ia]; const ItBox &A_ = box[a];
            if (!A_.h) continue;
            nb[a].push_back(a);
            for (int ib = ia + 1; ib < K; ++ib) {
                const int b = byc[ib]; const ItBox &B_ = box[b];
                if (B_.c0 >= A_.c0 + A_.w) break;
                if (!B_.h || B_.r0 >= A_.r0 + A_.h || A_.r0 >= B_.r0 + B_.h) continue;
                nb[a].push_back(b); nb[b].push_back(a);
            }
        }
    }
    std::vector<int> nptr((size_t)K + 1, 0), nidx, diag((size_t)K, -1);
    for (int k = 0; k < K; ++k) {
        std::sort(nb[k].begin(), nb[k].end());
        nptr[k] = (int)nidx.size();
        for (int j : nb[k]) { if (j == k) diag[k] = (int)nidx.size(); nidx.push_back(j); }
    }
    nptr[K] = (int)nidx.size();
    const int nn = (int)nidx.size();
    std::vector<int4> pairs;
    for (int k = 0; k < K; ++k)
        for (int q = nptr[k]; q < nptr[k + 1]; ++q) {
            const int j = nidx[q];
            if (j < k) continue;
            const int back = (int)(std::lower_bound(nidx.begin() + nptr[j], nidx.begin() + nptr[j + 1], k) - nidx.begin());
            pairs.push_back(make_int4(k, j, q, back));
        }
    ht.mark("boxes, passes, lists");
    // ---- device
    DevBuf *I = ctx->itp;
    DevBuf &dAcp = I[0], &dArow = I[1], &dAval = I[2], &dBox = I[3], &dPos = I[4], &dV64 = I[5], &dInv = I[6], &dScale = I[7], &dRptr = I[8], &dRk = I[9], &dRpos = I[10],
           &dPairs = I[11], &dAa64 = I[12], &dCp2 = I[13], &dErow2 = I[14], &dU2 = I[15], &dWhere = I[16], &dLvl = I[17], &dNvalRaw = I[18];
    DevBuf &dC = job ? job->dC : I[19], &dU = job ? job->dU : I[20], &dCraw = job ? job->dCraw : ctx->last_t.craw, &dNptr = job ? job->dNptr : I[21],
           &dNidx = job ? job->dNidx : I[22], &dNval = job ? job->dNval : I[23], &dAa = job ? job->dAa : I[24], &dWt = job ? job->dW : ctx->last_t.aa;
    if (!job) ctx->last_t.valid = false;
    const int64_t ldc = (T + 3) & ~int64_t(3);
    RET(to_dev(ctx, dAcp, A_colptr, (size_t)K + 1)); RET(to_dev(ctx, dArow, A_rowidx, (size_t)nnzA)); RET(to_dev(ctx, dAval, A_val, (size_t)nnzA));
    RET(to_dev(ctx, dBox, box)); RET(to_dev(ctx, dPos, pos)); RET(to_dev(ctx, dRptr, csr.rowptr)); RET(to_dev(ctx, dRk, csr.col.data(), (size_t)nnzt)); RET(to_dev(ctx, dRpos, rpos.data(), (size_t)nnzt));
    RET(to_dev(ctx, dPairs, pairs)); RET(to_dev(ctx, dCp2, colptr2)); RET(to_dev(ctx, dErow2, erow2.data(), (size_t)(2 * nnzt))); RET(to_dev(ctx, dWhere, where));
    RET(dV64.ensure((size_t)std::max<int64_t>(1, 2 * nnzt) * sizeof(double)));
    RET(dInv.ensure((size_t)K * sizeof(double))); RET(dScale.ensure((size_t)K * sizeof(double))); RET(dAa64.ensure((size_t)K * sizeof(double)));
    RET(dNvalRaw.ensure((size_t)std::max(1, nn) * sizeof(float)));
    RET(dU2.ensure((size_t)2 * K * ldc * sizeof(float)));
    RET(dU.ensure((size_t)K * ldc * sizeof(float))); RET(dC.ensure((size_t)K * ldc * sizeof(float))); RET(dCraw.ensure((size_t)K * ldc * sizeof(float)));
    CK(hipMemsetAsync(dCraw.p, 0, (size_t)K * ldc * sizeof(float), ctx->st()));                 // C_raw = zeros(K, T)  (HALS_temporal.m:45)
    CK(hipMemsetAsync(dAa64.p, 0, (size_t)K * sizeof(double), ctx->st()));                      // (a neuron without a box has no diagonal pair: aa = 0)
    const int ysplit = (int)std::max<int64_t>(1, std::min<int64_t>(16, 2048 / std::max<int32_t>(1, K)));
    LAUNCH(ctx, "init_temporal_filter", k_it_filter, dim3((unsigned)K, (unsigned)ysplit), dim3(256), 0, dAcp.as<int64_t>(), dArow.as<int>(), dAval.as<float>(), dBox.as<ItBox>(),
           dPos.as<int64_t>(), nr, nr_b, P->nc_b, roff, coff, P->p, P->ring_dr.as<int>(), P->ring_dc.as<int>(), P->W.as<float>(), d, dV64.as<double>());
    LAUNCH(ctx, "init_temporal_colsum", k_it_colred<false>, dim3((unsigned)K), dim3(256), 0, dV64.as<double>(), dBox.as<ItBox>(), dPos.as<int64_t>(), dInv.as<double>());
    LAUNCH(ctx, "init_temporal_winner", k_it_winner, dim3((unsigned)((d + 255) / 256)), dim3(256), 0, dRptr.as<int>(), dRk.as<int>(), dRpos.as<int>(), dBox.as<ItBox>(),
           dInv.as<double>(), (int)K, d, dV64.as<double>());
    LAUNCH(ctx, "init_temporal_colsq", k_it_colred<true>, dim3((unsigned)K), dim3(256), 0, dV64.as<double>(), dBox.as<ItBox>(), dPos.as<int64_t>(), dScale.as<double>());
    if (!pairs.empty())
        LAUNCH(ctx, "init_temporal_gram", k_it_gram, dim3((unsigned)pairs.size()), dim3(64), 0, dPairs.as<int4>(), dBox.as<ItBox>(), dPos.as<int64_t>(), dV64.as<double>(),
               dNvalRaw.as<float>(), dAa64.as<double>());
    DevBuf &dPixG = ctx->itp[28], &dOff = job ? job->dOff : ctx->itp[29];
    if (dopts) {
        RET(dPixG.ensure((size_t)d * sizeof(double))); RET(dOff.ensure((size_t)K * sizeof(double)));
        LAUNCH(ctx, "init_temporal_pixconst", k_it_pixconst, dim3((unsigned)((d + 255) / 256)), dim3(256), 0, P->ymean_d.as<double>(), P->W.as<float>(), d, nr, nr_b, P->nc_b, roff, coff,
               P->p, P->ring_dr.as<int>(), P->ring_dc.as<int>(), dPixG.as<double>());
        LAUNCH(ctx, "init_temporal_rowconst", k_it_rowconst, dim3((unsigned)K), dim3(256), 0, dV64.as<double>(), dBox.as<ItBox>(), dPos.as<int64_t>(), dPixG.as<double>(), nr,
               dAa64.as<double>(), dOff.as<double>());
    }
    // V and aa come back under the projection (nn + K numbers): the schedule follows the non-zeros of V
    std::vector<float> nval((size_t)std::max(1, nn));
    std::vector<double> aa64((size_t)K);
    if (nn) CK(hipMemcpyAsync(nval.data(), dNvalRaw.p, (size_t)nn * sizeof(float), hipMemcpyDeviceToHost, ctx->st()));
    CK(hipMemcpyAsync(aa64.data(), dAa64.p, (size_t)K * sizeof(double), hipMemcpyDeviceToHost, ctx->st()));
    int j0 = 0;
    for (int p = 0; p < npass; ++p) {                          // one launch set per pass; the video is read once unless a block is crowded
        const int j1 = pass_end[p];
        if (j1 > j0) {
            const int rcv = vproj_temporal(ctx, P, 2 * (j1 - j0), colptr2.data() + 2 * j0, erow2.data(), nullptr, dCp2.as<int64_t>() + 2 * j0, dErow2.as<int>(), nullptr,
                                           dU2.as<float>() + (int64_t)2 * j0 * ldc, ldc, dV64.as<double>(), false);
            if (rcv < 0) return rcv;
            if (rcv > 0) return fail(CNMFE_EUNSUPPORTED, "init_temporal: the projection's partial sums of %d columns x %lld frames do not fit", 2 * (j1 - j0), (long long)T);
        }
        j0 = j1;
    }
    LAUNCH(ctx, "init_temporal_split", k_it_split, dim3((unsigned)((ldc + 255) / 256), (unsigned)K), dim3(256), 0, dU2.as<float>(), dWhere.as<int>(), dScale.as<double>(), ldc, T,
           dU.as<float>(), dC.as<float>());
    ht.mark("filter, start, gram, projection queued");
    RET(ctx_check_errflag(ctx));                               // the wait for V
    ht.mark("wait for V (sync)");
    // the lists the sweeps read: the non-zeros of V only (a pair of boxes that meet where one of the two columns is 0 couples nothing)
    std::vector<char> upd((size_t)K, 0);
    std::vector<float> aa((size_t)K, 0.f);
    std::vector<std::vector<int>> nbv((size_t)K);
    std::vector<int> nptr2((size_t)K + 1, 0), nidx2; std::vector<float> nval2;
    for (int k = 0; k < K; ++k) {
        aa[k] = (float)aa64[k]; upd[k] = aa[k] > 0.f;          // ind_update = find(aa > 0)  (HALS_temporal.m:51)
        nptr2[k] = (int)nidx2.size();
        for (int q = nptr[k]; q < nptr[k + 1]; ++q)
            if (nval[q] != 0.f || nidx[q] == k) { nidx2.push_back(nidx[q]); nval2.push_back(nval[q]); nbv[k].push_back(nidx[q]); }
    }
    nptr2[K] = (int)nidx2.size();
    RET(to_dev(ctx, dNptr, nptr2)); RET(to_dev(ctx, dNidx, nidx2)); RET(to_dev(ctx, dNval, nval2)); RET(to_dev(ctx, dAa, aa)); RET(to_dev(ctx, dWt, AA));
    // ---- the sweeps
    const unsigned nthr = T >= 2048 ? 1024 : 256;
    auto plain = [&](int iters) -> int {
        if (iters <= 0) return 0;
        bool dag_on; std::vector<std::vector<int>> levels;
        it_schedule(ctx, K, nbv, upd, iters, false, &dag_on, levels);
        std::vector<int> flat, off;
        for (auto &l : levels) { off.push_back((int)flat.size()); flat.insert(flat.end(), l.begin(), l.end()); }
        ctx->last_nlevels = (int64_t)levels.size() * (dag_on ? 1 : iters);
        RET(to_dev(ctx, dLvl, flat));
        for (int it = 0; it < (dag_on ? 1 : iters); ++it)
            for (size_t l = 0; l < levels.size(); ++l)
                LAUNCH(ctx, "temporal_hals_level", k_hals_temporal, dim3((unsigned)levels[l].size()), dim3(nthr), 0, dLvl.as<int>() + off[l], dNptr.as<int>(), dNidx.as<int>(),
                       dNval.as<float>(), dAa.as<float>(), dU.as<float>(), dC.as<float>(), dCraw.as<float>(), ldc, T);
        return 0;
    };
    if (job) {
        // the first call's sweeps run here, on the patch's lane; the last iters_last are the job cnmfe_temporal_jobs_sweep runs with the other patches'
        RET(plain(iters_plain));
        bool dag_on; std::vector<std::vector<int>> levels;
        it_schedule(ctx, K, nbv, upd, iters_last, dopts != nullptr, &dag_on, levels);
        job->P = P; job->K = K; job->ldc = ldc; job->T = T; job->maxIter = iters_last; job->deconv = dopts != nullptr; job->swept = false; job->finished = true;
        job->diag.clear(); job->upd = upd; job->term_applied = false; job->nn = 0; job->levels = std::move(levels); job->dag = dag_on; job->has_w = true; job->has_off = dopts != nullptr;
        if (dopts) {
            job->dopts = *dopts;
            RET(job->dS.ensure((size_t)K * ldc * sizeof(float)));
            CK(hipMemsetAsync(job->dS.p, 0, (size_t)K * ldc * sizeof(float), ctx->st()));
            RET(job->dPars.ensure((size_t)K * sizeof(float))); RET(job->dSn.ensure((size_t)K * sizeof(float))); RET(job->dB.ensure((size_t)K * sizeof(float)));
            CK(hipMemsetAsync(job->dPars.p, 0, (size_t)K * sizeof(float), ctx->st()));           // kernel parameters estimated fresh (:168)
            CK(hipMemsetAsync(job->dSn.p, 0, (size_t)K * sizeof(float), ctx->st()));
        }
        if (AA_out) memcpy(AA_out, AA.data(), (size_t)K * sizeof(float));
        ht.mark("job queued");
        return 0;
    }
    if (!dopts) {
        RET(plain(iters_plain + iters_last));                  // twelve plain sweeps on the same U, V are one graph
        if (S_out || pars_out || sn_out) return fail(CNMFE_EINVAL, "init_temporal: S / kernel_pars / sn exist with deconvolution options only");
    } else {
        RET(plain(iters_plain));
        DevBuf &dS = I[25], &dPars = I[26], &dSn = I[27];
        RET(dS.ensure((size_t)K * ldc * sizeof(float)));
        CK(hipMemsetAsync(dS.p, 0, (size_t)K * ldc * sizeof(float), ctx->st()));
        RET(dPars.ensure((size_t)K * sizeof(float))); RET(dSn.ensure((size_t)K * sizeof(float)));
        CK(hipMemsetAsync(dPars.p, 0, (size_t)K * sizeof(float), ctx->st()));                    // kernel parameters estimated fresh (:168)
        CK(hipMemsetAsync(dSn.p, 0, (size_t)K * sizeof(float), ctx->st()));
        if (iters_last > 0) {
            bool dag_on; std::vector<std::vector<int>> levels;
            it_schedule(ctx, K, nbv, upd, iters_last, true, &dag_on, levels);
            std::vector<int> flat, off;
            for (auto &l : levels) { off.push_back((int)flat.size()); flat.insert(flat.end(), l.begin(), l.end()); }
            ctx->last_nlevels += (int64_t)levels.size() * (dag_on ? 1 : iters_last);
            RET(to_dev(ctx, dLvl, flat));
            RET(temporal_deconv_sweeps(ctx, dopts, T, K, dag_on ? -1 : iters_last, levels, dLvl.as<int>(), off, dC.as<float>(), dCraw.as<float>(), dS.as<float>(), ldc,
                                       dU.as<float>(), dNptr.as<int>(), dNidx.as<int>(), dNval.as<float>(), dAa.as<float>(), dPars.as<float>(), dSn.as<float>(), dOff.as<double>()));
        }
        RET(download_traces(ctx, dS.as<float>(), ldc, S_out, K, T, c_order));
        if (pars_out) CK(hipMemcpyAsync(pars_out, dPars.p, (size_t)K * sizeof(float), hipMemcpyDeviceToHost, ctx->st()));
        if (sn_out) CK(hipMemcpyAsync(sn_out, dSn.p, (size_t)K * sizeof(float), hipMemcpyDeviceToHost, ctx->st()));
    }
    ctx->last_t.set(K, ldc, T);                                // C_raw rows and AA stay on the device for cnmfe_stitch_add
    RET(download_traces(ctx, dC.as<float>(), ldc, C_out, K, T, c_order));
    RET(download_traces(ctx, dCraw.as<float>(), ldc, C_raw_out, K, T, c_order));
    if (AA_out) memcpy(AA_out, AA.data(), (size_t)K * sizeof(float));
    if (C_out || C_raw_out || S_out || pars_out || sn_out) RET(ctx_check_errflag(ctx));
    ht.mark("sweeps queued");
    return 0;
}
