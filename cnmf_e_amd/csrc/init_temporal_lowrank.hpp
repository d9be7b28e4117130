// (f) known footprints under background_model = 'svd': the traces of given footprints AND the temporal factors of a given spatial background on the resident video
//   @Sources2D/initTemporal.m:180-192 (svd branch) -> utilities/HALS_temporal.m:48-68 / :70-104 (the sweeps; no rough start, C is given)
//     b0 = mean(Ypatch, 2);   tmp_A = [A_patch, b];   tmp_C = (tmp_A' tmp_A) \ (tmp_A' Ypatch - tmp_A' b0 1');   C = tmp_C(1:k, :);   f = tmp_C(k+1:end, :);
//     Ypatch = Ypatch - (b f + b0);   [~, C] = HALS_temporal(Ypatch, A_patch, C, 10);   [~, C_raw] = HALS_temporal(Ypatch, A_patch, C, 2, deconv_options)
// Included by factor.hip behind init_temporal.hpp (its schedule, the level kernels and the deconvolving sweeps are reused as they are).
//
// Nothing of Ypatch - (b f + b0) is formed.  b0 is the pixel mean, so Ypatch - b0 is the resident CENTRED video Yc on the patch rows, and with M = [A_p, b]
// (A_p: A on the patch rows; n = k + nb columns) everything follows from  G = M' M  (n x n)  and  R = M' Yc  (n x T), both fp64:
//   k_itl_gram     G on the pairs of columns that can meet (footprints whose bounding boxes meet; every pair with a column of b), one workgroup per pair, fixed tree
//   k_itl_colconst  what the fp32 centring of the resident video left of the pixel means, per column of M (subtracted from the rows of R)
//   vproj_columns64  R in block-tiled passes over the video (vproj.hip: the fp64 panels and k_vp_proj_b of the temporal update, reduced WITHOUT a rounding to
//                  fp32); the columns of b ride in the same pass, one list slot in every block.  More than 64 columns over a 16 x 16 block: several passes
//                  (vproj_pass_plan), the counter init_temporal_lowrank_video_reads
//   host           G comes down (<= 2048^2 doubles), is Cholesky-factored in float64 -- a pivot <= n eps max(diag G) fails the call -- and goes back as 16 x 16 tiles
//                  in the operand order of v_mfma_f64_16x16x4_f64
//   k_itl_trsm     L Y = R, then L' X = Y: per 16 columns of T one wave walks the block rows; the off-diagonal panels are MFMAs (A operand: the -L tile, B operand:
//                  the solved rows), the 16-wide diagonal block is substituted from LDS, one column per lane.  No inverse is formed or multiplied with
//   k_itl_finish   C0 = X(1:k, :) (one rounding),  f = X(k+1:n, :) -> the patch's resident f,  U = R(1:k, :) - G(1:k, k+1:n) f = A_p' (Yc - b f)  (fp64, one rounding)
// then the sweeps of init_temporal_run on U, V = the non-zeros of G(1:k, 1:k) and aa = its diagonal, started from C0.  Yc - b f carries no constant per row, so
// GetSn of the deconvolving sweeps needs no offset (k_it_rowconst has no counterpart here).
// A column of b that is identically zero (G(i, i) = 0) is DECOUPLED: its pivot becomes 1, its row of f is exactly 0 and no other unknown changes by a bit (its row
// and column of G and its row of R are exact zeros).  The reference divides by a singular matrix there.
// No atomics; every reduction has a fixed order: two calls give the same bits.  A failed call writes nothing of the patch.

constexpr int ITL_NMAX = 2048;
typedef double itl_d4 __attribute__((ext_vector_type(4)));      // the accumulator of v_mfma_f64_16x16x4_f64

// value of the sorted column [a0, a1) at row q; a column that stores every row (a column of b) is indexed directly
__device__ __forceinline__ double itl_find(const int *__restrict__ row, const double *__restrict__ val, int64_t a0, int64_t a1, int q, int64_t d) {
    if (a1 - a0 == d) return val[a0 + q];
    int64_t lo = a0, hi = a1;
    while (lo < hi) { const int64_t mid = (lo + hi) >> 1; if (row[mid] < q) lo = mid + 1; else hi = mid; }
    return (lo < a1 && row[lo] == q) ? val[lo] : 0.0;
}
// pairs[i] = (a, b): G(a, b) = G(b, a) = sum over the entries of column a of M(., a) M(., b)
__global__ void __launch_bounds__(256) k_itl_gram(const int2 *__restrict__ pairs, const int64_t *__restrict__ cp, const int *__restrict__ row, const double *__restrict__ val,
                                                  int64_t d, int n, double *__restrict__ G) {
    __shared__ double red[256];
    const int2 pr = pairs[blockIdx.x];
    const int64_t a0 = cp[pr.x], a1 = cp[pr.x + 1], b0 = cp[pr.y], b1 = cp[pr.y + 1];
    double s = 0.0;
    for (int64_t e = a0 + threadIdx.x; e < a1; e += 256) s += val[e] * (pr.x == pr.y ? val[e] : itl_find(row, val, b0, b1, row[e], d));
    red[threadIdx.x] = s; __syncthreads();
    for (int o = 128; o > 0; o >>= 1) { if ((int)threadIdx.x < o) red[threadIdx.x] += red[threadIdx.x + o]; __syncthreads(); }
    if (threadIdx.x == 0) { G[(int64_t)pr.x * n + pr.y] = red[0]; G[(int64_t)pr.y * n + pr.x] = red[0]; }
}

// One triangular solve  Lop X = B  over all T columns; Lop = L (BACK = false: block rows top down) or L' (BACK = true: bottom up).  nt block rows of 16.
//   Lt[((i nt + j) 4 + kk) 64 + lane] = -Lop(16 i + (lane & 15), 16 j + 4 kk + (lane >> 4)): the A operand of MFMA kk of tile (i, j), one coalesced load per wave
//   Ld[(i 16 + r) 16 + c]             =  Lop(16 i + r, 16 i + c): the diagonal block
// Workgroup = 64 columns, a wave owns 16 (the N of the MFMA).  Block row i:  acc = B_i - sum_j Lop_ij X_j  -- acc: lane holds rows (lane >> 4) + 4 r, column
// lane & 15; B operand of MFMA kk: X(16 j + 4 kk + (lane >> 4), column lane & 15), read back from `out` (written by this workgroup only, behind a barrier) --
// then the 16 x 16 substitution out of LDS: lanes 0..15 take one column each.  in / out: nt * 16 rows of ld doubles, ld a multiple of 64; in != out.
template <bool BACK>
__global__ void __launch_bounds__(256) k_itl_trsm(const double *__restrict__ Lt, const double *__restrict__ Ld, int nt, const double *__restrict__ in, double *out, int64_t ld) {
    __shared__ double S[4][16][17];
    __shared__ double D[16][17];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, n = lane & 15, kq = lane >> 4;
    const int64_t col = ((int64_t)blockIdx.x * 4 + wave) * 16 + n;
    for (int s = 0; s < nt; ++s) {
        const int i = BACK ? nt - 1 - s : s;
        D[threadIdx.x >> 4][threadIdx.x & 15] = Ld[(int64_t)i * 256 + threadIdx.x];
        itl_d4 acc;
#pragma unroll
        for (int r = 0; r < 4; ++r) acc[r] = in[(int64_t)(16 * i + kq + 4 * r) * ld + col];
        for (int q = 0; q < s; ++q) {
            const int j = BACK ? nt - 1 - q : q;
            const double *lt = Lt + ((int64_t)i * nt + j) * 256 + lane;
            const double *x = out + (int64_t)(16 * j + kq) * ld + col;
            const double a0 = lt[0], a1 = lt[64], a2 = lt[128], a3 = lt[192];
            const double x0 = x[0], x1 = x[4 * ld], x2 = x[8 * ld], x3 = x[12 * ld];
            acc = __builtin_amdgcn_mfma_f64_16x16x4f64(a0, x0, acc, 0, 0, 0);
            acc = __builtin_amdgcn_mfma_f64_16x16x4f64(a1, x1, acc, 0, 0, 0);
            acc = __builtin_amdgcn_mfma_f64_16x16x4f64(a2, x2, acc, 0, 0, 0);
            acc = __builtin_amdgcn_mfma_f64_16x16x4f64(a3, x3, acc, 0, 0, 0);
        }
#pragma unroll
        for (int r = 0; r < 4; ++r) S[wave][kq + 4 * r][n] = acc[r];
        __syncthreads();
        if (lane < 16) {
            double y[16];
#pragma unroll
            for (int rr = 0; rr < 16; ++rr) {
                const int r = BACK ? 15 - rr : rr;
                double v = S[wave][r][lane];
#pragma unroll
                for (int cc = 0; cc < rr; ++cc) { const int c = BACK ? 15 - cc : cc; v -= D[r][c] * y[c]; }
                y[r] = v / D[r][r];
            }
            double *o = out + (int64_t)(16 * i) * ld + ((int64_t)blockIdx.x * 4 + wave) * 16 + lane;
#pragma unroll
            for (int r = 0; r < 16; ++r) o[(int64_t)r * ld] = y[r];
        }
        __syncthreads();                                       // the rows of X_i are visible to the workgroup's next block rows; S and D are free
    }
}

// The resident video is centred about the FP32 pixel mean (k_center4): Yc = Y - fl32(Ymean), so a row of Yc still has the mean dm(q) = Ymean(q) - fl32(Ymean(q)),
// 6e-8 of the baseline.  The reference's right-hand side is M'(Y - Ymean 1') = M' Yc - (M' dm) 1':  cst[j] = sum over column j of M(m, j) dm(q(m)), fixed tree.
// (Left in, the constant moves every row of f and of the start by G^-1 M' dm: 6e-9 of f on the test fixtures, where fp64 gives 1e-13.)
__global__ void __launch_bounds__(256) k_itl_colconst(const int64_t *__restrict__ cp, const int *__restrict__ row, const double *__restrict__ val, const double *__restrict__ ymean,
                                                      const float *__restrict__ ymean_f, int nr, int nr_b, int roff, int coff, double *__restrict__ cst) {
    __shared__ double red[256];
    const int j = blockIdx.x;
    double s = 0.0;
    for (int64_t e = cp[j] + threadIdx.x; e < cp[j + 1]; e += 256) {
        const int m = row[e];
        const int64_t q = (int64_t)(m / nr + coff) * nr_b + (m % nr + roff);
        s += val[e] * (ymean[q] - (double)ymean_f[q]);
    }
    red[threadIdx.x] = s; __syncthreads();
    for (int o = 128; o > 0; o >>= 1) { if ((int)threadIdx.x < o) red[threadIdx.x] += red[threadIdx.x + o]; __syncthreads(); }
    if (threadIdx.x == 0) cst[j] = red[0];
}

// C0(k, :) = X(k, :), U(k, :) = R(k, :) - sum_i G(k, K + i) X(K + i, :) for k < K (fp64, one rounding; 0 past T);  f(i, :) = X(K + i, :) for the nb rows behind
__global__ void __launch_bounds__(256) k_itl_finish(const double *__restrict__ R, const double *__restrict__ X, int64_t ldr, const double *__restrict__ G, int n, int K, int nb,
                                                    int64_t T, int64_t ldc, float *__restrict__ U, float *__restrict__ C, double *__restrict__ f) {
    const int j = blockIdx.y;
    const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (j >= K) { if (t < T) f[(int64_t)(j - K) * T + t] = X[(int64_t)j * ldr + t]; return; }
    if (t >= ldc) return;
    if (t >= T) { U[(int64_t)j * ldc + t] = 0.f; C[(int64_t)j * ldc + t] = 0.f; return; }
    double u = R[(int64_t)j * ldr + t];
    for (int i = 0; i < nb; ++i) u -= G[(int64_t)j * n + K + i] * X[(int64_t)(K + i) * ldr + t];
    U[(int64_t)j * ldc + t] = (float)u;
    C[(int64_t)j * ldc + t] = (float)X[(int64_t)j * ldr + t];
}
// b0(m) = Ymean of the patch pixel m
__global__ void __launch_bounds__(256) k_itl_b0(const double *__restrict__ ymean, int64_t d, int nr, int nr_b, int roff, int coff, double *__restrict__ b0) {
    const int64_t m = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (m >= d) return;
    b0[m] = ymean[(int64_t)((int)(m / nr) + coff) * nr_b + (int)(m % nr) + roff];
}

int init_temporal_lowrank_run(cnmfe_ctx *ctx, Patch *P, int patch_id, int32_t K, const int64_t *A_colptr, const int32_t *A_rowidx, const float *A_val, int32_t iters_plain,
                              int32_t iters_last, const cnmfe_deconv_opts *dopts, float *C_out, float *C_raw_out, float *S_out, float *pars_out, float *sn_out, float *AA_out,
                              double *f_out, double *b0_out, int c_order) {
    const int64_t T = P->T, d = P->d;
    const int nr = P->nr, nc = P->nc, nr_b = P->nr_b, roff = P->roff, coff = P->coff, nb = P->svd_nb;
    const int n = K + nb;
    if (!dopts && (S_out || pars_out || sn_out)) return fail(CNMFE_EINVAL, "init_temporal_lowrank: S / kernel_pars / sn exist with deconvolution options only");
    const int64_t nmax = std::min<int64_t>(ITL_NMAX, std::max<int64_t>(1, ctx->opt("init_temporal_lowrank_nmax", ITL_NMAX)));
    if (K > nmax) return fail(CNMFE_EUNSUPPORTED, "init_temporal_lowrank: patch %d: %d footprints alone exceed the %lld unknowns the joint system may have", patch_id, K, (long long)nmax);
    RET(ensure_ymean(ctx, P));
    HostTrace ht(ctx, "init_temporal_lowrank");
    // ---- host: M = [A on the patch rows, b] as CSC over PATCH rows; the footprints' bounding boxes
    std::vector<int64_t> mcp((size_t)n + 1, 0);
    std::vector<int32_t> mrow; std::vector<double> mval;
    std::vector<int4> bx((size_t)K);                          // (r0, c0, r1, c1) inclusive; r1 < r0: no entry on the patch
    mrow.reserve((size_t)A_colptr[K]); mval.reserve((size_t)A_colptr[K]);
    for (int32_t k = 0; k < K; ++k) {
        int4 b = make_int4(INT32_MAX, INT32_MAX, -1, -1);
        for (int64_t e = A_colptr[k]; e < A_colptr[k + 1]; ++e) {
            const int r = A_rowidx[e] % nr_b - roff, c = A_rowidx[e] / nr_b - coff;
            if (r < 0 || r >= nr || c < 0 || c >= nc) continue;                    // rows outside the patch are dropped (:103-109)
            mrow.push_back(c * nr + r); mval.push_back((double)A_val[e]);
            b.x = std::min(b.x, r); b.y = std::min(b.y, c); b.z = std::max(b.z, r); b.w = std::max(b.w, c);
        }
        bx[k] = b;
        mcp[k + 1] = (int64_t)mrow.size();
    }
    const int64_t nnzA = mcp[K];
    if (nnzA + (int64_t)nb * d >= (int64_t(1) << 31)) return fail(CNMFE_EUNSUPPORTED, "init_temporal_lowrank: nnz([A, b]) too large");
    mrow.resize((size_t)(nnzA + (int64_t)nb * d));
    for (int i = 0; i < nb; ++i) {
        int32_t *r = mrow.data() + nnzA + (int64_t)i * d;
        for (int64_t m = 0; m < d; ++m) r[m] = (int32_t)m;
        mcp[K + i + 1] = mcp[K + i] + d;
    }
    // the pairs of G: footprints whose boxes meet (k <= j), every footprint with every column of b, the columns of b among themselves
    std::vector<std::vector<int>> nbl((size_t)K);
    {
        std::vector<int> byc((size_t)K);
        for (int k = 0; k < K; ++k) byc[k] = k;
        std::sort(byc.begin(), byc.end(), [&](int a, int b) { return bx[a].y != bx[b].y ? bx[a].y < bx[b].y : a < b; });
        for (int ia = 0; ia < K; ++ia) {
            const int a = byc[ia]; const int4 &A_ = bx[a];
            if (A_.z < A_.x) continue;
            nbl[a].push_back(a);
            for (int ib = ia + 1; ib < K; ++ib) {
                const int b = byc[ib]; const int4 &B_ = bx[b];
                if (B_.z >= B_.x && B_.y > A_.w) break;
                if (B_.z < B_.x || B_.x > A_.z || A_.x > B_.z) continue;
                nbl[a].push_back(b); nbl[b].push_back(a);
            }
        }
    }
    std::vector<int2> pairs;
    for (int k = 0; k < K; ++k) {
        std::sort(nbl[k].begin(), nbl[k].end());
        for (int j : nbl[k]) if (j >= k) pairs.push_back(make_int2(k, j));
        if (bx[k].z >= bx[k].x) for (int i = 0; i < nb; ++i) pairs.push_back(make_int2(k, K + i));
    }
    for (int i = 0; i < nb; ++i) for (int j = i; j < nb; ++j) pairs.push_back(make_int2(K + i, K + j));
    // ---- the passes of the projection and the columns in pass order
    std::vector<int> pass_of;
    const int npass = vproj_pass_plan(P, n, mcp.data(), mrow.data(), 1, pass_of, 0);
    if (npass <= 0) return fail(CNMFE_EUNSUPPORTED, "init_temporal_lowrank: no pass plan for patch %d", patch_id);
    std::vector<int> order((size_t)n), pass_end((size_t)npass, 0);
    for (int j = 0; j < n; ++j) order[j] = j;
    std::stable_sort(order.begin(), order.end(), [&](int a, int b) { return pass_of[a] < pass_of[b]; });
    // (the projection wants a pass's columns consecutive: a second column-pointer list in pass order over the SAME entries -- colptr pairs (begin, end) do not
    // exist in this format, so the entries are permuted with their columns)
    std::vector<int64_t> ocp((size_t)n + 1, 0), ofrom((size_t)n);
    for (int jj = 0; jj < n; ++jj) { const int j = order[jj]; ofrom[jj] = mcp[j]; ocp[jj + 1] = ocp[jj] + (mcp[j + 1] - mcp[j]); pass_end[pass_of[j]] = jj + 1; }
    for (int p = 1; p < npass; ++p) pass_end[p] = std::max(pass_end[p], pass_end[p - 1]);
    bool identity = true;
    for (int jj = 0; jj < n; ++jj) if (order[jj] != jj) { identity = false; break; }
    std::vector<int32_t> orow;
    if (!identity) {
        orow.resize(mrow.size());
        for (int jj = 0; jj < n; ++jj) {
            const int64_t len = ocp[jj + 1] - ocp[jj];
            if (len) memcpy(&orow[ocp[jj]], &mrow[ofrom[jj]], (size_t)len * sizeof(int32_t));
        }
    }
    ht.mark("columns, pairs, passes");
    // ---- device
    DevBuf *I = ctx->itp, *Q = ctx->itl;
    DevBuf &dCp = Q[0], &dRow = Q[1], &dVal = Q[2], &dPairs = Q[3], &dG = Q[4], &dLt = Q[5], &dLd = Q[6], &dR = Q[7], &dY = Q[8], &dX = Q[9], &dOcp = Q[10], &dOrow = Q[11], &dOval = Q[12],
           &dRowOf = Q[13], &dCst = Q[14];
    DevBuf &dLvl = I[17], &dC = I[19], &dU = I[20], &dNptr = I[21], &dNidx = I[22], &dNval = I[23], &dAa = I[24];
    const int64_t ldc = (T + 3) & ~int64_t(3), ldr = (T + 63) & ~int64_t(63);
    const int nt = (n + 15) >> 4, n16 = nt * 16;
    const size_t mtot = (size_t)(nnzA + (int64_t)nb * d);
    RET(to_dev(ctx, dCp, mcp)); RET(to_dev(ctx, dRow, mrow.data(), mtot)); RET(dVal.ensure(std::max<size_t>(1, mtot) * sizeof(double)));
    if (nnzA) RET(to_dev(ctx, dVal, mval.data(), (size_t)nnzA));
    if (nb > 0) CK(hipMemcpyAsync(dVal.as<double>() + nnzA, P->svd_b.p, (size_t)nb * d * sizeof(double), hipMemcpyDeviceToDevice, ctx->st()));
    RET(to_dev(ctx, dPairs, pairs));
    RET(dG.ensure((size_t)n * n * sizeof(double)));
    CK(hipMemsetAsync(dG.p, 0, (size_t)n * n * sizeof(double), ctx->st()));
    if (!pairs.empty())
        LAUNCH(ctx, "itl_gram", k_itl_gram, dim3((unsigned)pairs.size()), dim3(256), 0, dPairs.as<int2>(), dCp.as<int64_t>(), dRow.as<int>(), dVal.as<double>(), d, n, dG.as<double>());
    RET(dCst.ensure((size_t)n * sizeof(double)));
    LAUNCH(ctx, "itl_colconst", k_itl_colconst, dim3((unsigned)n), dim3(256), 0, dCp.as<int64_t>(), dRow.as<int>(), dVal.as<double>(), P->ymean_d.as<double>(), P->ymean_f.as<float>(),
           nr, nr_b, roff, coff, dCst.as<double>());
    std::vector<double> G((size_t)n * n);
    CK(hipMemcpyAsync(G.data(), dG.p, (size_t)n * n * sizeof(double), hipMemcpyDeviceToHost, ctx->st()));
    hipEvent_t evG = nullptr;
    CK(hipEventCreateWithFlags(&evG, hipEventDisableTiming));
    struct EvGuard { hipEvent_t e; ~EvGuard() { (void)hipEventDestroy(e); } } evguard{evG};
    CK(hipEventRecord(evG, ctx->st()));
    // R = M' Yc, one launch set per pass, queued under the host's factorisation
    const int64_t *hcp = identity ? mcp.data() : ocp.data();
    const int32_t *hrow = identity ? mrow.data() : orow.data();
    const int64_t *dcp_ = dCp.as<int64_t>(); const int *drow_ = dRow.as<int>(); const double *dval_ = dVal.as<double>();
    if (!identity) {
        // the permuted copy on the device: rows from the host, values gathered column by column on the device (the columns of b never visit the host)
        RET(to_dev(ctx, dOcp, ocp)); RET(to_dev(ctx, dOrow, orow.data(), mtot)); RET(dOval.ensure(std::max<size_t>(1, mtot) * sizeof(double)));
        for (int jj = 0; jj < n; ++jj) {
            const int64_t len = ocp[jj + 1] - ocp[jj];
            if (len) CK(hipMemcpyAsync(dOval.as<double>() + ocp[jj], dVal.as<double>() + ofrom[jj], (size_t)len * sizeof(double), hipMemcpyDeviceToDevice, ctx->st()));
        }
        dcp_ = dOcp.as<int64_t>(); drow_ = dOrow.as<int>(); dval_ = dOval.as<double>();
    }
    RET(to_dev(ctx, dRowOf, order));
    RET(dR.ensure((size_t)n16 * ldr * sizeof(double))); RET(dY.ensure((size_t)n16 * ldr * sizeof(double))); RET(dX.ensure((size_t)n16 * ldr * sizeof(double)));
    CK(hipMemsetAsync(dR.p, 0, (size_t)n16 * ldr * sizeof(double), ctx->st()));                  // (the rows behind n: zero right-hand sides of unit pivots)
    int reads = 0;
    for (int p = 0, j0 = 0; p < npass; ++p) {
        const int j1 = pass_end[p];
        if (j1 > j0) {
            const int rcv = vproj_columns64(ctx, P, j1 - j0, hcp + j0, hrow, dcp_ + j0, drow_, dval_, dRowOf.as<int>() + j0, dCst.as<double>(), dR.as<double>(), ldr);
            if (rcv < 0) return rcv;
            if (rcv > 0) return fail(CNMFE_EUNSUPPORTED, "init_temporal_lowrank: the projection's partial sums of %d columns x %lld frames do not fit", j1 - j0, (long long)T);
            ++reads;
        }
        j0 = j1;
    }
    ht.mark("gram, projection queued");
    // ---- host: Cholesky of G in float64 (row by row: every inner product runs over two contiguous rows)
    CK(hipEventSynchronize(evG));
    const auto tf0 = std::chrono::steady_clock::now();
    double dmax = 0.0; int nbz = 0;
    for (int i = 0; i < nb; ++i) if (G[(size_t)(K + i) * n + K + i] == 0.0) { G[(size_t)(K + i) * n + K + i] = 1.0; ++nbz; }   // an all-zero column of b: decoupled
    if (n - nbz > nmax) return fail(CNMFE_EUNSUPPORTED, "init_temporal_lowrank: patch %d: the joint system has %d unknowns (at most %lld)", patch_id, n - nbz, (long long)nmax);
    for (int i = 0; i < n; ++i) dmax = std::max(dmax, G[(size_t)i * n + i]);
    const double thr = (double)(n - nbz) * 2.220446049250313e-16 * dmax;
    std::vector<double> Lh((size_t)n16 * n16, 0.0);
    for (int i = n; i < n16; ++i) Lh[(size_t)i * n16 + i] = 1.0;
    for (int i = 0; i < n; ++i) {
        double *Li = &Lh[(size_t)i * n16];
        for (int j = 0; j <= i; ++j) {
            const double *Lj = &Lh[(size_t)j * n16];
            double s = G[(size_t)i * n + j];
            for (int k = 0; k < j; ++k) s -= Li[k] * Lj[k];
            if (j < i) Li[j] = s / Lj[j];
            else {
                if (!(s > thr)) return fail(CNMFE_ESTATE, "init_temporal_lowrank: patch %d: [A, b]'[A, b] is singular to working precision: Cholesky pivot %d is %.3g (threshold %.3g)%s",
                                            patch_id, i, s, thr, i < K ? "" : " (a column of b)");
                Li[i] = std::sqrt(s);
            }
        }
    }
    std::vector<double> Lt((size_t)nt * nt * 256, 0.0), Ld((size_t)2 * nt * 256);
    for (int i = 0; i < nt; ++i) {
        for (int r = 0; r < 16; ++r) for (int c = 0; c < 16; ++c) {
            const double v = Lh[(size_t)(16 * i + r) * n16 + 16 * i + c];
            Ld[((size_t)i * 16 + r) * 16 + c] = v;                             // forward: L_ii
            Ld[((size_t)(nt + i) * 16 + c) * 16 + r] = v;                      // backward: L_ii'
        }
        for (int j = 0; j < nt; ++j) {
            if (j == i) continue;
            double *t = &Lt[((size_t)i * nt + j) * 256];
            for (int kk = 0; kk < 4; ++kk) for (int lane = 0; lane < 64; ++lane) {
                const int rr = 16 * i + (lane & 15), cc = 16 * j + 4 * kk + (lane >> 4);
                t[kk * 64 + lane] = j < i ? -Lh[(size_t)rr * n16 + cc] : -Lh[(size_t)cc * n16 + rr];      // (j > i: L'(rr, cc) = L(cc, rr))
            }
        }
    }
    ctx->itl_factor_us = (int64_t)std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - tf0).count();
    ht.mark("wait for G, factorisation");
    // the lists the sweeps read: the non-zeros of V = fl32(G(1:k, 1:k)); aa = its diagonal (:160 is the same sum on the patch)
    std::vector<char> upd((size_t)K, 0);
    std::vector<float> aa((size_t)K, 0.f);
    std::vector<std::vector<int>> nbv((size_t)K);
    std::vector<int> nptr2((size_t)K + 1, 0), nidx2; std::vector<float> nval2;
    for (int k = 0; k < K; ++k) {
        aa[k] = (float)G[(size_t)k * n + k]; upd[k] = aa[k] > 0.f;
        nptr2[k] = (int)nidx2.size();
        for (int j : nbl[k]) {
            const float v = (float)G[(size_t)k * n + j];
            if (v != 0.f || j == k) { nidx2.push_back(j); nval2.push_back(v); nbv[k].push_back(j); }
        }
    }
    nptr2[K] = (int)nidx2.size();
    // ---- from here on the call cannot fail for a reason of its input: the patch's state changes
    DevBuf &dCraw = ctx->last_t.craw, &dWt = ctx->last_t.aa;
    ctx->last_t.valid = false;
    P->residual.invalidate();                                  // f and b0 change: whatever Ysig holds is no longer the residual under them
    RET(to_dev(ctx, dLt, Lt)); RET(to_dev(ctx, dLd, Ld));
    const unsigned gx = (unsigned)(ldr / 64);
    LAUNCH(ctx, "itl_trsm_forward", k_itl_trsm<false>, dim3(gx), dim3(256), 0, dLt.as<double>(), dLd.as<double>(), nt, dR.as<double>(), dY.as<double>(), ldr);
    LAUNCH(ctx, "itl_trsm_backward", k_itl_trsm<true>, dim3(gx), dim3(256), 0, dLt.as<double>(), dLd.as<double>() + (size_t)nt * 256, nt, dY.as<double>(), dX.as<double>(), ldr);
    RET(dU.ensure((size_t)K * ldc * sizeof(float))); RET(dC.ensure((size_t)K * ldc * sizeof(float))); RET(dCraw.ensure((size_t)K * ldc * sizeof(float)));
    CK(hipMemsetAsync(dCraw.p, 0, (size_t)K * ldc * sizeof(float), ctx->st()));                  // C_raw = zeros(K, T)  (HALS_temporal.m:45)
    LAUNCH(ctx, "itl_finish", k_itl_finish, dim3((unsigned)((std::max(ldc, T) + 255) / 256), (unsigned)n), dim3(256), 0, dR.as<double>(), dX.as<double>(), ldr, dG.as<double>(), n, (int)K, nb,
           T, ldc, dU.as<float>(), dC.as<float>(), P->svd_f.as<double>());
    LAUNCH(ctx, "itl_b0", k_itl_b0, dim3((unsigned)((d + 255) / 256)), dim3(256), 0, P->ymean_d.as<double>(), d, nr, nr_b, roff, coff, P->svd_b0.as<double>());
    ctx->itl_reads = reads;
    RET(to_dev(ctx, dNptr, nptr2)); RET(to_dev(ctx, dNidx, nidx2)); RET(to_dev(ctx, dNval, nval2)); RET(to_dev(ctx, dAa, aa)); RET(to_dev(ctx, dWt, aa));
    // ---- the sweeps (init_temporal_run's, on this U, V and start)
    const unsigned nthr = T >= 2048 ? 1024 : 256;
    ctx->last_nlevels = 0;
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
    if (!dopts) RET(plain(iters_plain + iters_last));          // twelve plain sweeps on the same U, V are one graph
    else {
        RET(plain(iters_plain));
        DevBuf &dS = I[25], &dPars = I[26], &dSn = I[27];
        RET(dS.ensure((size_t)K * ldc * sizeof(float)));
        CK(hipMemsetAsync(dS.p, 0, (size_t)K * ldc * sizeof(float), ctx->st()));
        RET(dPars.ensure((size_t)K * sizeof(float))); RET(dSn.ensure((size_t)K * sizeof(float)));
        CK(hipMemsetAsync(dPars.p, 0, (size_t)K * sizeof(float), ctx->st()));                    // kernel parameters estimated fresh
        CK(hipMemsetAsync(dSn.p, 0, (size_t)K * sizeof(float), ctx->st()));
        if (iters_last > 0) {
            bool dag_on; std::vector<std::vector<int>> levels;
            it_schedule(ctx, K, nbv, upd, iters_last, true, &dag_on, levels);
            std::vector<int> flat, off;
            for (auto &l : levels) { off.push_back((int)flat.size()); flat.insert(flat.end(), l.begin(), l.end()); }
            ctx->last_nlevels += (int64_t)levels.size() * (dag_on ? 1 : iters_last);
            RET(to_dev(ctx, dLvl, flat));
            RET(temporal_deconv_sweeps(ctx, dopts, T, K, dag_on ? -1 : iters_last, levels, dLvl.as<int>(), off, dC.as<float>(), dCraw.as<float>(), dS.as<float>(), ldc,
                                       dU.as<float>(), dNptr.as<int>(), dNidx.as<int>(), dNval.as<float>(), dAa.as<float>(), dPars.as<float>(), dSn.as<float>(), nullptr));
        }
        RET(download_traces(ctx, dS.as<float>(), ldc, S_out, K, T, c_order));
        if (pars_out) CK(hipMemcpyAsync(pars_out, dPars.p, (size_t)K * sizeof(float), hipMemcpyDeviceToHost, ctx->st()));
        if (sn_out) CK(hipMemcpyAsync(sn_out, dSn.p, (size_t)K * sizeof(float), hipMemcpyDeviceToHost, ctx->st()));
    }
    ctx->last_t.set(K, ldc, T);                                // C_raw rows and AA stay on the device for cnmfe_stitch_add
    RET(download_traces(ctx, dC.as<float>(), ldc, C_out, K, T, c_order));
    RET(download_traces(ctx, dCraw.as<float>(), ldc, C_raw_out, K, T, c_order));
    if (AA_out) memcpy(AA_out, aa.data(), (size_t)K * sizeof(float));
    if (f_out && nb > 0) CK(hipMemcpyAsync(f_out, P->svd_f.p, (size_t)nb * T * sizeof(double), hipMemcpyDeviceToHost, ctx->st()));
    if (b0_out) CK(hipMemcpyAsync(b0_out, P->svd_b0.p, (size_t)d * sizeof(double), hipMemcpyDeviceToHost, ctx->st()));
    RET(ctx_check_errflag(ctx));                               // one wait: the patch's new f and b0 are in place when the call returns
    ht.mark("solve, sweeps");
    return 0;
}
