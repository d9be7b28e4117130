// cnmfe_mex.cpp -- thin MEX gateway over the C ABI of include/cnmfe.h (one command string per entry point).
//
// Build where MATLAB is installed (not built in this repository: the image has no MATLAB; tests/test_host_logic.py only syntax-checks this
// file against the stub headers in tests/mex_stub/):
//     mex -O -largeArrayDims cnmfe_mex.cpp -I../../../include -L../.. -lcnmfe_hip
// House conventions follow the reference's own MEX (ca_source_extraction/utilities/graph_conn_comp_mex.cpp:38-64, 88, 115): argument checks
// first, mexErrMsgIdAndTxt on failure, outputs allocated with mxCreate*, inputs never written, scratch from mxMalloc.
//
// mexErrMsgIdAndTxt does not return (it long-jumps out of the MEX function), so NO C++ object with a destructor is alive at any point that can
// fail: every temporary is mxMalloc memory, which MATLAB releases itself when a MEX function exits through an error.
//
//   h = cnmfe_mex('create', device)                                        cnmfe_mex('destroy', h)
//   cnmfe_mex('patch', h, pid, patch_pos, block_pos, d1, d2, T)            distribute_data.m:165-171 rectangles
//   cnmfe_mex('upload', h, pid, Yblock, t0)                                Yblock: d_b x nt of class single / double / uint16 / uint8
//   cnmfe_mex('ring_init', h, pid, radius, num_neighbors)                  get_nhood.m + initComponents_parallel.m:213-236
//   [Wt, b0] = cnmfe_mex('get_ring', h, pid, d, d_b)                       W{m}.' (d_b x d sparse) and b0{m}
//   cnmfe_mex('set_ring', h, pid, Wt, b0)                                  put a W{m}, b0{m} of an earlier session back on the device
//   f = cnmfe_mex('first_run', h, pid)                                     update_background_parallel.m:143
//   cnmfe_mex('bind_traces', h, C)                                         obj.C once per iteration; later C arguments may be int32 ROW INDICES into it
//   info = cnmfe_mex('fit_ring', h, pid, A_block, C_or_rows, with_projection)             fit_ring_model.m:1
//   info = cnmfe_mex('fit_ring_ssub', h, pid, fit_pid, res_pid, bg_ssub, A_block, C_or_rows, with_projection)
//   cnmfe_mex('derive', h, pid, new_pid, bg_ssub, 'nearest' | 'bicubic')
//   cnmfe_mex('residual', h, pid, A_prev_block, C_or_rows)                 update_spatial_parallel.m:162-166 (result stays on the device)
//   cnmfe_mex('residual_ssub', h, pid, res_pid, bg_ssub, A_prev_block, C_or_rows)
//   sn = cnmfe_mex('get_sn', h, pid, d)                                    update_sn = true
//   cnmfe_mex('set_noise', h, pid, sn_block);  sn_block = cnmfe_mex('estimate_noise', h, pid, d_b, nframes)
//   cnmfe_mex('background_ssub', ...), cnmfe_mex('compute_rss_ssub', ...), cnmfe_mex('reconstruct_background_ssub', ...)   bg_ssub > 1
//   A = cnmfe_mex('spatial', h, pid, alg, A_patch, C_or_rows, IND_patch, sn, param)       HALS_spatial*.m / nnls_spatial.m
//   [C, C_raw, aa] = cnmfe_mex('temporal', h, pid, A_patch, C_or_rows, maxIter)           HALS_temporal.m:1 (fewer outputs: fewer downloads)
//   [C, C_raw, S, pars, sn, aa] = cnmfe_mex('temporal_deconv', h, pid, A, C, maxIter, smin, max_tau, pars)
//   [C_raw, aa] = cnmfe_mex('fast_temporal', h, pid, A, T)
//   cnmfe_mex('stitch_begin', h, K, T);  cnmfe_mex('stitch_add', h, ind)   update_temporal_parallel.m:269-278, on the device
//   C_raw = cnmfe_mex('stitch_temporal', hs, subtract_min, K, T)           :279-286 over the contexts hs (one per GPU; RCCL all-reduce)
//   [C, C_raw, S, pars, sn] = cnmfe_mex('deconv_temporal', h, C_raw, smin, max_tau)       deconvTemporal.m:29-105
//   rss = cnmfe_mex('compute_rss', h, pid, A_patch, C_or_rows, b0_block, b0_new_patch)
//   Ybg = cnmfe_mex('reconstruct_background', h, pid, b0_block, b0_new_patch, frame0, nframes)
//   keep = cnmfe_mex('postprocess', h, A, d1, d2)                          post_process_spatial.m:19-32 (connected)
//   [box, off, out, host_col] = cnmfe_mex('circular_constraints', h, A, d1, d2)                  circular_constraints.m:8-55 per column (compactSpatial)
//   [box, off, out, host_col] = cnmfe_mex('search_dilate', h, A, d1, d2, se, nb, nrgthr)         determine_search_location(A, 'dilate', ...) with the element se
//   [keep, ind_small, host_col] = cnmfe_mex('trim_spatial', h, A, d1, d2, thr, sz, min_pixel)    Sources2D.m:942-965 (trimSpatial)
// Round 6 -- the calls the measured host (cnmf_e_amd/sources2d.py, bench.py) makes and this gateway lacked; the .m twins use them:
//   cnmfe_mex('set_option', h, name, value)                                cnmfe_set_option (the tunables of include/cnmfe.h; the defaults ARE the fast path)
//   cnmfe_mex('synchronize', h)                                            wait for the context's stream; reports what its kernels raised
//   q = cnmfe_mex('spatial_queue', h, pid, alg, A_patch, C_or_rows, IND_patch, sn, param)   the update is QUEUED (sweeps + the copy of the result into pinned
//   A = cnmfe_mex('spatial_collect', h, q)                                 memory) and collected later: patch m + 1 is set up and queued while patch m runs
//   job = cnmfe_mex('temporal_job', h, pid, A_patch, C_or_rows, maxIter)   everything of 'temporal' up to the Gauss-Seidel sweeps; 'temporal_jobs_sweep' then runs
//   cnmfe_mex('temporal_jobs_sweep', h)                                    level l of EVERY job in one launch; cnmfe_mex('stitch_add_job', h, job, ind) adds a job
//   cnmfe_mex('stitch_finish_async', h, subtract_min, K, T)                :279-286 + bind on one context without waiting; C_raw = cnmfe_mex('stitch_collect', h)
// Seed images (correlation_pnr_parallel.m:70-104 per patch):
//   [Cn_block, PNR_block] = cnmfe_mex('seed_images', h, pid, psf, nframes, Q)   psf: odd n x n (or []), Q: nframes x M orthonormal detrend basis (or [] / omitted);
//                                                                          nr_b x nc_b double images of the block (its size is remembered from 'patch')
//   [Cn_ds, PNR_ds] = cnmfe_mex('seed_images_ds', h, pid, ssub, tsub, psf, nframes, Q)        the seed images of dsData(block): ceil(nr_b / ssub) x ceil(nc_b / ssub), Q: floor(nframes / tsub) x M
// Greedy initialisation, a peel session per patch (greedyROI_endoscope.m:119-145, 287-311, 378-402; the search loop is the host's):
//   [Cn_ds, PNR_ds, Sn_ds, Yds] = cnmfe_mex('peel_open_ds', h, pid, ssub, tsub, psf, nframes, Qpre)   the session on dsData(block); Qpre: nframes x M, the full-length basis; Yds single, d1s d2s x Ts
//   [Cn_block, PNR_block, Sn_block] = cnmfe_mex('peel_open', h, pid, psf, nframes, Q)          the arguments and images of 'seed_images' (+ GetSn of the filtered traces)
//   [corr, ai, ci, stats] = cnmfe_mex('peel_extract', h, pid, r, c, gSiz)                       (r, c): the seed, 1-BASED in the block; corr, ai: the clipped
//                                                                          (2 gSiz + 1)^2 box; ci: 1 x nframes; stats: [max(diff(y0)) std(diff(y0)) norm(ci) GetSn(ci) n_hi n_lo]
//   [PNR_box2, Cn_box2] = cnmfe_mex('peel_apply', h, pid, r, c, gSiz, ai, Hai, ci, sig, min_pnr, min_corr)   Hai: the clipped (4 gSiz + 1)^2 box
//   cnmfe_mex('peel_close', h, pid)
//   [Cn_patch, PNR_patch, Sn_patch, Yres] = cnmfe_mex('peel_open_residual', h, pid, A_patch, C_or_rows, psf)   the second pass (initComponents_residual_parallel.m:186-220):
//                                                                          the session on the PATCH and on Ysig - A_patch C, after 'residual' / 'residual_ssub'; the images are
//                                                                          nr x nc of the patch, Yres (asked for as 4th output) d x T single; extract / apply then take the seed in the patch
//   [Cn_ds, PNR_ds, Sn_ds, Yds] = cnmfe_mex('peel_open_residual_ds', h, pid, ssub, tsub, A_patch, C_or_rows, psf)   the second pass with options.ssub / options.tsub: the session on
//                                                                          dsData(Ysig - A_patch C) of the PATCH, ceil(nr / ssub) x ceil(nc / ssub) pixels, Ts = floor(T / tsub) frames; A_patch
//                                                                          at full resolution; Yds (asked for as 4th output) d1s d2s x Ts single; extract / apply then take the seed on that grid
// Known footprints (@Sources2D/initTemporal.m:156-168 per patch; the loop over the patches, the stitch and deconvTemporal are the caller's, as in cnmf_e_amd/sources2d.py -- no .m twin is written):
//   [C, C_raw, AA, S, pars, sn] = cnmfe_mex('init_temporal', h, pid, A_block, iters_plain, iters_last, smin, max_tau)   A_block: sparse, BLOCK rows x K; without smin and
//                                                                          max_tau the last sweeps are plain too (three outputs).  C_raw and AA also stay on the device:
//                                                                          cnmfe_mex('stitch_add', h, ind) then adds AA .* C_raw (:285)
// Merging (merge_high_corr.m:50-85,172-196,236 and its two siblings, Sources2D.m:1683-1715; the K x K criteria and the groups are the caller's).  A trace SOURCE is the
// last argument: a K x T matrix (uploaded), or 'bound' | 'craw' | 's' | 'diff' followed by K, T -- the context's own C, C_raw, S, the last 'trace_diff_spikes':
//   cnmfe_mex('traces_load', h, C, C_raw, S, kernel_pars)                  the object's matrices become the context's ([] for what it lacks); not needed after 'deconv' on the bound matrix
//   R = cnmfe_mex('trace_corr', h, raw, source...)                         corr(X') (raw = 1: X * X') as K x K double
//   [sn, S_] = cnmfe_mex('trace_diff_spikes', h, source...)                the S-less branch (:57-66); the result stays on the device as the source 'diff'
//   q = cnmfe_mex('trace_tags', h, K)                                      K x 4: max(C), std(C_raw - C), GetSn(C_raw), spikes after frame 1
//   [C, C_raw, S, pars, sn] = cnmfe_mex('merge_apply', h, grp_ptr, grp_idx, w, keep, T, smin, max_tau)   merged traces, their deconvolution, obj.delete: on the device
// Batch mode (demo_batch_1p.m:120-142; the batch methods are cnmf_e_amd/batch.py's -- no .m twin is written):
//   e = cnmfe_mex('trace_energy', h, source...)                            sum(X.^2, 2) as K x 1 double: a batch's weights in the footprint average (update_spatial_batch.m:29)
//   cnmfe_mex('traces_grow', h, K_new)                                     C = [C; zeros(K_new - K, T)] on the bound matrix (and the residents that belong to it), on the device
// dF/F (Sources2D.m:540-570, extract_DF_F_endoscope; the loop over the patches is the caller's, as in cnmf_e_amd/sources2d.py -- no .m twin is written):
//   cnmfe_mex('df_begin', h, K, T)                                         the K x T fp64 accumulator of (A ./ sum(A.^2, 1))' * Ybg, zeroed
//   cnmfe_mex('df_add_background', h, pid, b0_block, b0_new_patch, A_patch, ind)   all frames of one patch, after 'residual' (as 'reconstruct_background'); ind: 1-based rows
//   cnmfe_mex('df_add_background_ssub', h, pid, b0_new_patch, A_patch, ind)        the same after 'background_ssub'
//   cnmfe_mex('df_add_frames', h, Ybg, frame0, A, ind)                     a d x nframes slab of a background the caller holds
//   Yf = cnmfe_mex('df_fetch', h);  cnmfe_mex('df_load', h, Yf)            the accumulator to / from the host (a sharded run's all-reduce goes in between)
//   [C_df, C_raw_df, Df, Yf] = cnmfe_mex('df_finish', h, inv_norm, df_prctile, df_window, C, C_raw)   C, C_raw: K x T matrices or 'bound' / 'craw'; df_window 0 / []: none
// Closing calls (Sources2D.m:573-653 orderROIs, show_demixed_video.m; the methods are cnmf_e_amd/sources2d.py's -- no .m twin is written):
//   q = cnmfe_mex('trace_order_stats', h, K)                               K x 7: mean(C), var(C), var(C_raw - C), max(C), ||C_raw||_2, ||C_raw||_1, max(C_raw)
//   [raw, bg, signal, denoised, residual, mixed] = cnmfe_mex('demix_frames', h, pid, b0_block, b0_new_patch, A_patch, CC, ind, col, mix_scale, frame0, stride, nframes)
//   [...] = cnmfe_mex('demix_frames_ssub', h, pid, b0_new_patch, A_patch, CC, ind, col, mix_scale, frame0, stride, nframes)     the panels of the displayed frames of one patch
#include "mex.h"
#include "matrix.h"
#include <string.h>
#include <stdint.h>
#include "cnmfe.h"

#define MAX_CTX 64
static cnmfe_ctx *g_ctx[MAX_CTX];
static int g_nctx = 0;
// queued spatial updates ('spatial_queue' ... 'spatial_collect'): the ticket of the copy into pinned memory and a persistent copy of the mask whose pattern the result has
#define MAX_PEND 1024
typedef struct { int used; cnmfe_ctx *c; int64_t ticket; float *pinned; int64_t nnz; mxArray *ind; } Pending;
static Pending g_pend[MAX_PEND];
// the asynchronous stitch of a context ('stitch_finish_async' ... 'stitch_collect'): K x T floats, row-major, pinned
typedef struct { float *pinned; size_t K, T; } StitchOut;
static StitchOut g_stitch[MAX_CTX];
// block sizes by (context, patch id), noted by 'patch': what 'seed_images' shapes its outputs with
#define MAX_DIMS 4096
typedef struct { cnmfe_ctx *c; int pid; int32_t nr_b, nc_b, nr_p, nc_p, peel_nr, peel_nc; int64_t T, peel_n; } BlockDims;   // peel_n, peel_nr, peel_nc: frames and geometry of the open peel session ('peel_open': the block, 'peel_open_residual': the patch)
static BlockDims g_dims[MAX_DIMS];
static int g_ndims = 0;
static void at_exit(void) {
    g_ndims = 0;
    for (int i = 0; i < MAX_PEND; ++i) if (g_pend[i].used) { if (g_pend[i].pinned) cnmfe_host_free(g_pend[i].pinned); if (g_pend[i].ind) mxDestroyArray(g_pend[i].ind); g_pend[i].used = 0; }
    for (int i = 0; i < MAX_CTX; ++i) if (g_stitch[i].pinned) { cnmfe_host_free(g_stitch[i].pinned); g_stitch[i].pinned = NULL; }
    for (int i = 0; i < g_nctx; ++i) if (g_ctx[i]) { cnmfe_destroy(g_ctx[i]); g_ctx[i] = NULL; }
    g_nctx = 0;
}
#define FAIL(...) mexErrMsgIdAndTxt("cnmfe_mex:error", __VA_ARGS__)
#define CHECK(rc) do { if ((rc) != 0) FAIL("%s", cnmfe_last_error()); } while (0)

static cnmfe_ctx *ctx_of(const mxArray *h) {
    const double v = mxGetScalar(h);
    const int i = (int)v;
    if (i < 1 || i > g_nctx || !g_ctx[i - 1]) FAIL("invalid context handle");
    return g_ctx[i - 1];
}
// ---- plain-data views of MATLAB arrays (all storage mxMalloc'ed) ----
typedef struct { int32_t K; int64_t nnz; int64_t *cp; int32_t *ri; float *v; } Csc;
static Csc csc_of(const mxArray *A) {                       // sparse / full, double / logical -> int64 colptr, int32 rowidx, float values
    Csc o; o.K = 0; o.nnz = 0; o.ri = NULL; o.v = NULL;
    if (mxIsEmpty(A)) { o.cp = (int64_t *)mxCalloc(1, sizeof(int64_t)); return o; }
    mxArray *S = NULL; const mxArray *src = A;
    if (!mxIsSparse(A)) { mxArray *in = (mxArray *)A; if (mexCallMATLAB(1, &S, 1, &in, "sparse")) FAIL("sparse() failed"); src = S; }
    if (!mxIsDouble(src) && !mxIsLogical(src)) FAIL("sparse matrices must be double or logical");
    o.K = (int32_t)mxGetN(src);
    const mwIndex *jc = mxGetJc(src), *ir = mxGetIr(src);
    o.nnz = (int64_t)jc[o.K];
    o.cp = (int64_t *)mxMalloc(((size_t)o.K + 1) * sizeof(int64_t));
    o.ri = (int32_t *)mxMalloc(((size_t)o.nnz + 1) * sizeof(int32_t));
    o.v = (float *)mxMalloc(((size_t)o.nnz + 1) * sizeof(float));
    for (int32_t k = 0; k <= o.K; ++k) o.cp[k] = (int64_t)jc[k];
    if (mxIsLogical(src)) { for (int64_t e = 0; e < o.nnz; ++e) { o.ri[e] = (int32_t)ir[e]; o.v[e] = 1.f; } }
    else { const double *pr = mxGetPr(src); for (int64_t e = 0; e < o.nnz; ++e) { o.ri[e] = (int32_t)ir[e]; o.v[e] = (float)pr[e]; } }
    if (S) mxDestroyArray(S);
    return o;
}
static float *f32_of(const mxArray *M, size_t *n_out) {     // single / double -> float copy
    const size_t n = mxGetNumberOfElements(M);
    float *o = (float *)mxMalloc((n + 1) * sizeof(float));
    if (mxIsSingle(M)) memcpy(o, mxGetData(M), n * sizeof(float));
    else if (mxIsDouble(M)) { const double *p = mxGetPr(M); for (size_t i = 0; i < n; ++i) o[i] = (float)p[i]; }
    else FAIL("expected a single or double array");
    if (n_out) *n_out = n;
    return o;
}
// a trace argument: a K x T single / double matrix (column-major, uploaded) or an int32 vector of 1-based rows of the bound matrix
typedef struct { const float *ptr; int order; } Traces;
static Traces traces_of(const mxArray *C, int32_t K) {
    Traces t; t.ptr = NULL; t.order = CNMFE_COLMAJOR;
    if (K == 0) return t;
    if (mxIsInt32(C)) {
        if ((int32_t)mxGetNumberOfElements(C) != K) FAIL("row list has %d entries for %d footprints", (int)mxGetNumberOfElements(C), (int)K);
        int32_t *rows = (int32_t *)mxMalloc((size_t)K * sizeof(int32_t));
        const int32_t *src = (const int32_t *)mxGetData(C);
        for (int32_t k = 0; k < K; ++k) rows[k] = src[k] - 1;
        t.ptr = (const float *)rows; t.order = CNMFE_BOUND_ROWS;
        return t;
    }
    if ((int32_t)mxGetM(C) != K) FAIL("trace matrix has %d rows for %d footprints", (int)mxGetM(C), (int)K);
    t.ptr = f32_of(C, NULL);
    return t;
}
static int32_t *ind_of(const mxArray *I, size_t *n_out) {      // 1-based rows (double or int32) -> 0-based int32
    const size_t n = mxGetNumberOfElements(I);
    int32_t *ind = (int32_t *)mxMalloc((n + 1) * sizeof(int32_t));
    if (mxIsInt32(I)) { const int32_t *s = (const int32_t *)mxGetData(I); for (size_t i = 0; i < n; ++i) ind[i] = s[i] - 1; }
    else if (mxIsDouble(I)) { const double *s = mxGetPr(I); for (size_t i = 0; i < n; ++i) ind[i] = (int32_t)s[i] - 1; }
    else FAIL("row lists must be double or int32");
    *n_out = n;
    return ind;
}
static mxArray *to_double(const float *v, size_t r, size_t c) {
    mxArray *o = mxCreateDoubleMatrix(r, c, mxREAL);
    double *p = mxGetPr(o);
    for (size_t i = 0; i < r * c; ++i) p[i] = v[i];
    return o;
}
static mxArray *info_of(const int64_t info[4]) {
    mxArray *o = mxCreateDoubleMatrix(1, 4, mxREAL);
    for (int i = 0; i < 4; ++i) mxGetPr(o)[i] = (double)info[i];
    return o;
}
static void deconv_opts_of(cnmfe_deconv_opts *o, double smin, double max_tau) {
    memset(o, 0, sizeof(*o));
    o->type = 1; o->method = 1; o->smin = smin; o->max_tau = max_tau; o->optimize_b = 1; o->optimize_pars = 1; o->maxIter = 10;
}

void mexFunction(int nout, mxArray *pout[], int nin, const mxArray *pin[]) {
    if (nin < 1 || !mxIsChar(pin[0])) FAIL("first argument must be a command string");
    char cmd[40];
    if (mxGetString(pin[0], cmd, sizeof(cmd))) FAIL("command string too long");
    mexAtExit(at_exit);
    if (!strcmp(cmd, "create")) {
        if (g_nctx >= MAX_CTX) FAIL("too many contexts");
        cnmfe_ctx *c = cnmfe_create(nin > 1 ? (int)mxGetScalar(pin[1]) : 0);
        if (!c) FAIL("%s", cnmfe_last_error());
        g_ctx[g_nctx++] = c;
        pout[0] = mxCreateDoubleScalar((double)g_nctx);
        return;
    }
    if (nin < 2) FAIL("missing context handle");
    if (!strcmp(cmd, "stitch_temporal")) {                      // C_raw = cnmfe_mex('stitch_temporal', hs, subtract_min, K, T)   (single, K x T)
        if (nin != 5) FAIL("stitch_temporal: 5 inputs required (hs, subtract_min, K, T)");
        const int n = (int)mxGetNumberOfElements(pin[1]);
        if (n < 1 || n > MAX_CTX) FAIL("stitch_temporal: 1..%d context handles", MAX_CTX);
        cnmfe_ctx *cs[MAX_CTX];
        const double *hv = mxGetPr(pin[1]);
        for (int i = 0; i < n; ++i) { const int k = (int)hv[i]; if (k < 1 || k > g_nctx || !g_ctx[k - 1]) FAIL("invalid context handle"); cs[i] = g_ctx[k - 1]; }
        const size_t K = (size_t)mxGetScalar(pin[3]), T = (size_t)mxGetScalar(pin[4]);
        for (int i = 0; i < n; ++i) {                            // the engine writes stitch_K x stitch_T floats: the output is sized from ITS record, the caller's K, T are only checked
            int32_t Ks = 0; int64_t Ts = 0;
            CHECK(cnmfe_stitch_dims(cs[i], &Ks, &Ts));
            if ((size_t)Ks != K || (size_t)Ts != T) FAIL("stitch_temporal: K x T = %d x %d, but context %d accumulates %d x %d (stitch_begin)", (int)K, (int)T, i + 1, (int)Ks, (int)Ts);
        }
        pout[0] = mxCreateNumericMatrix(K, T, mxSINGLE_CLASS, mxREAL);
        CHECK(cnmfe_stitch_temporal(cs, n, mxGetScalar(pin[2]) != 0, nout > 0 ? (float *)mxGetData(pout[0]) : NULL, CNMFE_COLMAJOR));
        return;
    }
    cnmfe_ctx *c = ctx_of(pin[1]);
    if (!strcmp(cmd, "destroy")) {
        const int i = (int)mxGetScalar(pin[1]);
        int keep = 0;                                               // the block sizes noted for this context go with it (its address may be handed out again)
        for (int k = 0; k < g_ndims; ++k) if (g_dims[k].c != c) g_dims[keep++] = g_dims[k];
        g_ndims = keep;
        cnmfe_destroy(c); g_ctx[i - 1] = NULL; return;
    }
    if (!strcmp(cmd, "bind_traces")) {
        if (nin != 3) FAIL("bind_traces: 3 inputs required");
        if (mxIsEmpty(pin[2])) { CHECK(cnmfe_traces_bind(c, 0, 0, NULL, CNMFE_COLMAJOR)); return; }
        float *Cm = f32_of(pin[2], NULL);
        CHECK(cnmfe_traces_bind(c, (int32_t)mxGetM(pin[2]), (int64_t)mxGetN(pin[2]), Cm, CNMFE_COLMAJOR));
        return;
    }
    if (!strcmp(cmd, "stitch_begin")) {
        if (nin != 4) FAIL("stitch_begin: 4 inputs required (h, K, T)");
        CHECK(cnmfe_stitch_begin(c, (int32_t)mxGetScalar(pin[2]), (int64_t)mxGetScalar(pin[3])));
        return;
    }
    if (!strcmp(cmd, "stitch_add")) {                           // ind: 1-based rows (double or int32)
        if (nin != 3) FAIL("stitch_add: 3 inputs required (h, ind)");
        const size_t n = mxGetNumberOfElements(pin[2]);
        int32_t *ind = (int32_t *)mxMalloc((n + 1) * sizeof(int32_t));
        if (mxIsInt32(pin[2])) { const int32_t *s = (const int32_t *)mxGetData(pin[2]); for (size_t i = 0; i < n; ++i) ind[i] = s[i] - 1; }
        else if (mxIsDouble(pin[2])) { const double *s = mxGetPr(pin[2]); for (size_t i = 0; i < n; ++i) ind[i] = (int32_t)s[i] - 1; }
        else FAIL("stitch_add: ind must be double or int32");
        CHECK(cnmfe_stitch_add(c, (int32_t)n, ind));
        return;
    }
    if (!strcmp(cmd, "deconv_temporal")) {                      // [C, C_raw, S, pars, sn] = cnmfe_mex('deconv_temporal', h, C_raw, smin, max_tau)
        if (nin != 5) FAIL("deconv_temporal: 5 inputs required");
        const size_t K = mxGetM(pin[2]), T = mxGetN(pin[2]);
        float *Cr = f32_of(pin[2], NULL);
        cnmfe_deconv_opts o; deconv_opts_of(&o, mxGetScalar(pin[3]), mxGetScalar(pin[4]));
        float *Co = (float *)mxMalloc((K * T + 1) * sizeof(float)), *S = (float *)mxMalloc((K * T + 1) * sizeof(float));
        float *kp = (float *)mxMalloc((K + 1) * sizeof(float)), *sn = (float *)mxMalloc((K + 1) * sizeof(float));
        CHECK(cnmfe_deconv_temporal(c, (int32_t)K, (int64_t)T, Cr, CNMFE_COLMAJOR, &o, Co, S, kp, sn));
        pout[0] = to_double(Co, K, T);
        if (nout > 1) pout[1] = to_double(Cr, K, T);
        if (nout > 2) pout[2] = to_double(S, K, T);
        if (nout > 3) pout[3] = to_double(kp, K, 1);
        if (nout > 4) pout[4] = to_double(sn, K, 1);
        return;
    }
    // ---- merging (cnmfe.h section (h)).  A trace SOURCE is the last argument: a K x T single / double matrix (uploaded), or one of the names 'bound', 'craw', 's',
    // 'diff' followed by K, T (the context's own matrices: nothing is uploaded)
    if (!strcmp(cmd, "trace_corr") || !strcmp(cmd, "trace_diff_spikes")) {
        // R = cnmfe_mex('trace_corr', h, raw, X)  |  cnmfe_mex('trace_corr', h, raw, name, K, T)                       (K x K double)
        // [sn, S_] = cnmfe_mex('trace_diff_spikes', h, X)  |  cnmfe_mex('trace_diff_spikes', h, name, K, T)           (K x 1, K x T double)
        const int corr = !strcmp(cmd, "trace_corr"), a0 = corr ? 3 : 2;
        if (nin != a0 + 1 && nin != a0 + 3) FAIL("%s: the source is a matrix, or a name followed by K, T", cmd);
        size_t K, T; const float *X = NULL; int src = CNMFE_COLMAJOR;
        if (mxIsChar(pin[a0])) {
            char nm[16];
            if (nin != a0 + 3 || mxGetString(pin[a0], nm, sizeof(nm))) FAIL("%s: a named source needs K, T", cmd);
            src = !strcmp(nm, "bound") ? CNMFE_BOUND : !strcmp(nm, "craw") ? CNMFE_RES_CRAW : !strcmp(nm, "s") ? CNMFE_RES_S : !strcmp(nm, "diff") ? CNMFE_RES_DIFF : -1;
            if (src < 0) FAIL("%s: unknown source '%s' (bound, craw, s, diff)", cmd, nm);
            K = (size_t)mxGetScalar(pin[a0 + 1]); T = (size_t)mxGetScalar(pin[a0 + 2]);
        } else {
            if (nin != a0 + 1) FAIL("%s: too many inputs behind a matrix source", cmd);
            K = mxGetM(pin[a0]); T = mxGetN(pin[a0]); X = f32_of(pin[a0], NULL);
        }
        if (corr) {
            pout[0] = mxCreateDoubleMatrix(K, K, mxREAL);
            CHECK(cnmfe_trace_corr(c, (int32_t)K, (int64_t)T, X, src, mxGetScalar(pin[2]) != 0, mxGetPr(pout[0])));      // (symmetric: row-major is column-major)
            return;
        }
        float *sn = (float *)mxCalloc(K + 1, sizeof(float)), *S_ = (float *)mxCalloc(K * T + 1, sizeof(float));
        CHECK(cnmfe_trace_diff_spikes(c, (int32_t)K, (int64_t)T, X, src, sn, nout > 1 ? S_ : NULL));
        pout[0] = to_double(sn, K, 1);
        if (nout > 1) { pout[1] = mxCreateDoubleMatrix(K, T, mxREAL); double *p = mxGetPr(pout[1]); for (size_t k = 0; k < K; ++k) for (size_t t = 0; t < T; ++t) p[k + t * K] = S_[k * T + t]; }
        return;
    }
    if (!strcmp(cmd, "traces_load")) {                          // cnmfe_mex('traces_load', h, C, C_raw, S, kernel_pars): [] for a matrix the object does not have
        if (nin != 6) FAIL("traces_load: 6 inputs required (h, C, C_raw, S, kernel_pars)");
        const size_t K = mxGetM(pin[2]), T = mxGetN(pin[2]);
        for (int a = 3; a <= 4; ++a) if (!mxIsEmpty(pin[a]) && (mxGetM(pin[a]) != K || mxGetN(pin[a]) != T)) FAIL("traces_load: C_raw and S must have the shape of C");
        if (!mxIsEmpty(pin[5]) && mxGetNumberOfElements(pin[5]) != K) FAIL("traces_load: kernel_pars must have one entry per trace");
        CHECK(cnmfe_traces_load(c, (int32_t)K, (int64_t)T, f32_of(pin[2], NULL), mxIsEmpty(pin[3]) ? NULL : f32_of(pin[3], NULL), mxIsEmpty(pin[4]) ? NULL : f32_of(pin[4], NULL),
                                mxIsEmpty(pin[5]) ? NULL : f32_of(pin[5], NULL), CNMFE_COLMAJOR));
        return;
    }
    if (!strcmp(cmd, "trace_tags")) {                           // q = cnmfe_mex('trace_tags', h, K): K x 4 double = [max(C), std(C_raw - C), GetSn(C_raw), #spikes after frame 1]
        if (nin != 3) FAIL("trace_tags: 3 inputs required (h, K)");
        const size_t K = (size_t)mxGetScalar(pin[2]);
        double *q = (double *)mxCalloc(4 * K + 1, sizeof(double));
        CHECK(cnmfe_trace_tags(c, (int32_t)K, q));
        pout[0] = mxCreateDoubleMatrix(K, 4, mxREAL);
        for (size_t k = 0; k < K; ++k) for (int j = 0; j < 4; ++j) mxGetPr(pout[0])[k + j * K] = q[4 * k + j];
        return;
    }
    if (!strcmp(cmd, "trace_order_stats")) {                    // q = cnmfe_mex('trace_order_stats', h, K): K x 7 double = [mean(C), var(C), var(C_raw - C), max(C), norm(C_raw, 2), norm(C_raw, 1), max(C_raw)] per row
        if (nin != 3) FAIL("trace_order_stats: 3 inputs required (h, K)");
        const size_t K = (size_t)mxGetScalar(pin[2]);
        double *q = (double *)mxCalloc(7 * K + 1, sizeof(double));
        CHECK(cnmfe_trace_order_stats(c, (int32_t)K, q));
        pout[0] = mxCreateDoubleMatrix(K, 7, mxREAL);
        for (size_t k = 0; k < K; ++k) for (int j = 0; j < 7; ++j) mxGetPr(pout[0])[k + j * K] = q[7 * k + j];
        return;
    }
    if (!strcmp(cmd, "trace_energy")) {
        // e = cnmfe_mex('trace_energy', h, X)  |  cnmfe_mex('trace_energy', h, name, K, T): sum(X.^2, 2) as K x 1 double (update_spatial_batch.m:29)
        if (nin != 3 && nin != 5) FAIL("trace_energy: the source is a matrix, or a name followed by K, T");
        size_t K, T; const float *X = NULL; int src = CNMFE_COLMAJOR;
        if (mxIsChar(pin[2])) {
            char nm[16];
            if (nin != 5 || mxGetString(pin[2], nm, sizeof(nm))) FAIL("trace_energy: a named source needs K, T");
            src = !strcmp(nm, "bound") ? CNMFE_BOUND : !strcmp(nm, "craw") ? CNMFE_RES_CRAW : !strcmp(nm, "s") ? CNMFE_RES_S : !strcmp(nm, "diff") ? CNMFE_RES_DIFF : -1;
            if (src < 0) FAIL("trace_energy: unknown source '%s' (bound, craw, s, diff)", nm);
            K = (size_t)mxGetScalar(pin[3]); T = (size_t)mxGetScalar(pin[4]);
        } else {
            if (nin != 3) FAIL("trace_energy: too many inputs behind a matrix source");
            K = mxGetM(pin[2]); T = mxGetN(pin[2]); X = f32_of(pin[2], NULL);
        }
        pout[0] = mxCreateDoubleMatrix(K, 1, mxREAL);
        CHECK(cnmfe_trace_energy(c, (int32_t)K, (int64_t)T, X, src, mxGetPr(pout[0])));
        return;
    }
    if (!strcmp(cmd, "traces_grow")) {                          // cnmfe_mex('traces_grow', h, K_new): zero rows under the bound matrix and its residents, on the device
        if (nin != 3) FAIL("traces_grow: 3 inputs required (h, K_new)");
        CHECK(cnmfe_traces_grow(c, (int32_t)mxGetScalar(pin[2])));
        return;
    }
    if (!strcmp(cmd, "merge_apply")) {
        // [C, C_raw, S, kernel_pars, sn] = cnmfe_mex('merge_apply', h, grp_ptr, grp_idx, w, keep, T, smin, max_tau): grp_ptr = offsets 0 .. n of the groups in grp_idx / w
        // (numel = groups + 1, or [] for a plain delete), grp_idx and keep 1-based rows, T = frames of the context's matrices
        if (nin != 9) FAIL("merge_apply: 9 inputs required (h, grp_ptr, grp_idx, w, keep, T, smin, max_tau)");
        for (int a = 2; a <= 5; ++a) if (!mxIsEmpty(pin[a]) && !mxIsDouble(pin[a])) FAIL("merge_apply: index and weight vectors must be double");
        int64_t Tb = 0;
        if (cnmfe_get_option(c, "bound_T", &Tb) != 0 || (double)Tb != mxGetScalar(pin[6])) FAIL("merge_apply: T = %d, but the context's matrices have %d frames", (int)mxGetScalar(pin[6]), (int)Tb);   // (the outputs are sized with it)
        const size_t np_ = mxGetNumberOfElements(pin[2]), ng = np_ ? np_ - 1 : 0, n = mxGetNumberOfElements(pin[3]), nk = mxGetNumberOfElements(pin[5]), T = (size_t)mxGetScalar(pin[6]);
        if (mxGetNumberOfElements(pin[4]) != n) FAIL("merge_apply: one weight per group member");
        int32_t *gp = (int32_t *)mxCalloc(ng + 2, sizeof(int32_t)), *gi = (int32_t *)mxCalloc(n + 1, sizeof(int32_t)), *kp_ = (int32_t *)mxCalloc(nk + 1, sizeof(int32_t));
        for (size_t i = 0; i < np_; ++i) gp[i] = (int32_t)mxGetPr(pin[2])[i];
        if (ng && (size_t)gp[ng] != n) FAIL("merge_apply: grp_ptr must end at numel(grp_idx)");
        for (size_t i = 0; i < n; ++i) gi[i] = (int32_t)mxGetPr(pin[3])[i] - 1;
        for (size_t i = 0; i < nk; ++i) kp_[i] = (int32_t)mxGetPr(pin[5])[i] - 1;
        cnmfe_deconv_opts o; deconv_opts_of(&o, mxGetScalar(pin[7]), mxGetScalar(pin[8]));
        float *M[3];
        for (int j = 0; j < 3; ++j) M[j] = (float *)mxCalloc(nk * T + 1, sizeof(float));
        float *kp = (float *)mxCalloc(nk + 1, sizeof(float)), *sn = (float *)mxCalloc(nk + 1, sizeof(float));
        CHECK(cnmfe_merge_apply(c, (int32_t)ng, gp, gi, n ? mxGetPr(pin[4]) : NULL, (int32_t)nk, kp_, &o, M[0], M[1], M[2], kp, sn));
        for (int j = 0; j < 3 && j < (nout > 0 ? nout : 1); ++j) {
            pout[j] = mxCreateDoubleMatrix(nk, T, mxREAL);
            double *p = mxGetPr(pout[j]);
            for (size_t k = 0; k < nk; ++k) for (size_t t = 0; t < T; ++t) p[k + t * nk] = M[j][k * T + t];
        }
        if (nout > 3) pout[3] = to_double(kp, nk, 1);
        if (nout > 4) pout[4] = to_double(sn, nk, 1);
        return;
    }
    // ---- dF/F (cnmfe.h section (i)): the accumulator's K x T is the context's (cnmfe_df_dims) -- every output is sized from it, never from the caller
    if (!strcmp(cmd, "df_begin")) {                             // cnmfe_mex('df_begin', h, K, T)
        if (nin != 4) FAIL("df_begin: 4 inputs required (h, K, T)");
        CHECK(cnmfe_df_begin(c, (int32_t)mxGetScalar(pin[2]), (int64_t)mxGetScalar(pin[3])));
        return;
    }
    if (!strcmp(cmd, "df_add_frames")) {                        // cnmfe_mex('df_add_frames', h, Ybg, frame0, A, ind): Ybg d x nframes (a slab of reconstruct_background), frame0 0-based, ind 1-based rows
        if (nin != 6) FAIL("df_add_frames: 6 inputs required (h, Ybg, frame0, A, ind)");
        const size_t d = mxGetM(pin[2]), nf = mxGetN(pin[2]);
        Csc A = csc_of(pin[4]);
        if (A.K && mxGetM(pin[4]) != d) FAIL("df_add_frames: A has %d rows, Ybg %d", (int)mxGetM(pin[4]), (int)d);
        size_t n = 0;
        int32_t *ind = ind_of(pin[5], &n);
        if (n != (size_t)A.K) FAIL("df_add_frames: one accumulator row per column of A");
        CHECK(cnmfe_df_add_frames(c, (int64_t)d, (int64_t)mxGetScalar(pin[3]), (int64_t)nf, f32_of(pin[2], NULL), CNMFE_HOST, A.K, A.cp, A.ri, A.v, ind));
        return;
    }
    if (!strcmp(cmd, "df_fetch")) {                             // Yf = cnmfe_mex('df_fetch', h): the K x T accumulator (double)
        if (nin != 2) FAIL("df_fetch: 2 inputs required");
        int32_t Kd = 0; int64_t Td = 0;
        CHECK(cnmfe_df_dims(c, &Kd, &Td));
        const size_t K = (size_t)Kd, T = (size_t)Td;
        double *buf = (double *)mxCalloc(K * T + 1, sizeof(double));
        CHECK(cnmfe_df_fetch(c, buf));
        pout[0] = mxCreateDoubleMatrix(K, T, mxREAL);
        for (size_t k = 0; k < K; ++k) for (size_t t = 0; t < T; ++t) mxGetPr(pout[0])[k + t * K] = buf[k * T + t];
        return;
    }
    if (!strcmp(cmd, "df_load")) {                              // cnmfe_mex('df_load', h, Yf): a K x T double matrix becomes the accumulator (after the caller's all-reduce)
        if (nin != 3) FAIL("df_load: 3 inputs required (h, Yf)");
        if (!mxIsDouble(pin[2]) || mxIsSparse(pin[2])) FAIL("df_load: Yf must be a full double matrix");
        const size_t K = mxGetM(pin[2]), T = mxGetN(pin[2]);
        double *buf = (double *)mxCalloc(K * T + 1, sizeof(double));
        for (size_t k = 0; k < K; ++k) for (size_t t = 0; t < T; ++t) buf[k * T + t] = mxGetPr(pin[2])[k + t * K];
        CHECK(cnmfe_df_load(c, (int32_t)K, (int64_t)T, buf));
        return;
    }
    if (!strcmp(cmd, "df_finish")) {
        // [C_df, C_raw_df, Df, Yf] = cnmfe_mex('df_finish', h, inv_norm, df_prctile, df_window, C, C_raw): C and C_raw are K x T matrices (uploaded) or the names
        // 'bound' / 'craw' (the context's own); df_window = 0 or [] for none.  C_df, C_raw_df single, Df (K x 1, or K x T with a window) and Yf double
        if (nin != 7) FAIL("df_finish: 7 inputs required (h, inv_norm, df_prctile, df_window, C, C_raw)");
        int32_t Kd = 0; int64_t Td = 0;
        CHECK(cnmfe_df_dims(c, &Kd, &Td));
        const size_t K = (size_t)Kd, T = (size_t)Td;
        if (!mxIsDouble(pin[2]) || mxGetNumberOfElements(pin[2]) != K) FAIL("df_finish: inv_norm must hold %d doubles", (int)K);
        const int64_t w = mxIsEmpty(pin[4]) ? 0 : (int64_t)mxGetScalar(pin[4]);
        const float *X[2] = {NULL, NULL}; int src[2] = {CNMFE_COLMAJOR, CNMFE_COLMAJOR};
        for (int a = 0; a < 2; ++a) {
            const mxArray *M = pin[5 + a];
            if (mxIsChar(M)) {
                char nm[16];
                if (mxGetString(M, nm, sizeof(nm))) FAIL("df_finish: bad source name");
                src[a] = !strcmp(nm, "bound") ? CNMFE_BOUND : !strcmp(nm, "craw") ? CNMFE_RES_CRAW : -1;
                if (src[a] < 0) FAIL("df_finish: unknown source '%s' (bound, craw)", nm);
            } else {
                if (mxGetM(M) != K || mxGetN(M) != T) FAIL("df_finish: C and C_raw must be %d x %d", (int)K, (int)T);
                if (K) X[a] = f32_of(M, NULL);
            }
        }
        const int win = w > 0 && w <= Td;
        float *o0 = (float *)mxCalloc(K * T + 1, sizeof(float)), *o1 = (float *)mxCalloc(K * T + 1, sizeof(float));
        double *df = (double *)mxCalloc((win ? K * T : K) + 1, sizeof(double)), *yf = nout > 3 ? (double *)mxCalloc(K * T + 1, sizeof(double)) : NULL;
        CHECK(cnmfe_df_finish(c, mxGetPr(pin[2]), mxGetScalar(pin[3]), w, X[0], src[0], X[1], src[1], o0, o1, df, yf));
        float *o[2] = {o0, o1};
        for (int j = 0; j < 2 && j < (nout > 0 ? nout : 1); ++j) {
            pout[j] = mxCreateNumericMatrix(K, T, mxSINGLE_CLASS, mxREAL);
            float *p = (float *)mxGetData(pout[j]);
            for (size_t k = 0; k < K; ++k) for (size_t t = 0; t < T; ++t) p[k + t * K] = o[j][k * T + t];
        }
        if (nout > 2) {
            pout[2] = mxCreateDoubleMatrix(K, win ? T : 1, mxREAL);
            if (win) { for (size_t k = 0; k < K; ++k) for (size_t t = 0; t < T; ++t) mxGetPr(pout[2])[k + t * K] = df[k * T + t]; }
            else for (size_t k = 0; k < K; ++k) mxGetPr(pout[2])[k] = df[k];
        }
        if (nout > 3) { pout[3] = mxCreateDoubleMatrix(K, T, mxREAL); for (size_t k = 0; k < K; ++k) for (size_t t = 0; t < T; ++t) mxGetPr(pout[3])[k + t * K] = yf[k * T + t]; }
        return;
    }
    if (!strcmp(cmd, "postprocess")) {
        if (nin != 5) FAIL("postprocess: 5 inputs required");
        Csc A = csc_of(pin[2]);
        uint8_t *keep = (uint8_t *)mxCalloc((size_t)A.nnz + 1, 1);
        CHECK(cnmfe_post_process_spatial(c, (int32_t)mxGetScalar(pin[3]), (int32_t)mxGetScalar(pin[4]), A.K, A.cp, A.ri, A.v, keep));
        pout[0] = mxCreateLogicalMatrix((size_t)A.nnz, 1);
        mxLogical *k = mxGetLogicals(pout[0]);
        for (int64_t i = 0; i < A.nnz; ++i) k[i] = keep[i] != 0;
        return;
    }
    // footprint image operations (include/cnmfe.h): both calls of a boxed operation -- the sizes, then the result -- are made here.  box: 4 x K, rows (r0, c0, h, w)
    // with r0, c0 1-BASED; off: (K + 1) x 1, 0-based cell offsets into out; out: the cells of the boxes, column-major box after box; host_col: the columns left to the caller
    if (!strcmp(cmd, "circular_constraints") || !strcmp(cmd, "search_dilate")) {
        const bool dil = cmd[0] == 's';
        if (nin != (dil ? 8 : 5)) FAIL("%s: %d inputs required", cmd, dil ? 8 : 5);
        Csc A = csc_of(pin[2]);
        const int32_t d1 = (int32_t)mxGetScalar(pin[3]), d2 = (int32_t)mxGetScalar(pin[4]);
        const size_t K = (size_t)A.K;
        int32_t *box = (int32_t *)mxCalloc(4 * K + 4, sizeof(int32_t));
        int64_t *off = (int64_t *)mxCalloc(K + 1, sizeof(int64_t));
        uint8_t *hc = (uint8_t *)mxCalloc(K + 1, 1), *se = NULL;
        int32_t sh = 0, sw = 0, nb = 0; double nrgthr = 0;
        if (dil) {
            sh = (int32_t)mxGetM(pin[5]); sw = (int32_t)mxGetN(pin[5]); nb = (int32_t)mxGetScalar(pin[6]); nrgthr = mxGetScalar(pin[7]);
            if (!mxIsLogical(pin[5]) && !mxIsDouble(pin[5])) FAIL("search_dilate: se is a logical or double matrix");
            se = (uint8_t *)mxCalloc((size_t)sh * sw + 1, 1);
            for (int32_t i = 0; i < sh; ++i) for (int32_t j = 0; j < sw; ++j)                                  // column-major -> row-major
                se[(size_t)i * sw + j] = mxIsLogical(pin[5]) ? mxGetLogicals(pin[5])[i + (size_t)j * sh] != 0 : mxGetPr(pin[5])[i + (size_t)j * sh] != 0;
        }
        void *out = NULL;
        for (int pass = 0; pass < 2; ++pass) {
            const int64_t cap = pass ? off[K] : 0;
            if (pass) { if (cap == 0) break; out = mxCalloc((size_t)cap, dil ? 1 : sizeof(float)); }
            if (dil) CHECK(cnmfe_search_dilate(c, d1, d2, A.K, A.cp, A.ri, A.v, se, sh, sw, nb, nrgthr, box, off, (uint8_t *)out, cap, hc, CNMFE_HOST));
            else CHECK(cnmfe_circular_constraints(c, d1, d2, A.K, A.cp, A.ri, A.v, box, off, (float *)out, cap, hc, CNMFE_HOST));
        }
        pout[0] = mxCreateDoubleMatrix(4, K, mxREAL);
        for (size_t k = 0; k < K; ++k) for (int j = 0; j < 4; ++j) mxGetPr(pout[0])[4 * k + j] = (double)box[4 * k + j] + (j < 2 && box[4 * k + 2] > 0 ? 1.0 : 0.0);
        if (nout > 1) { pout[1] = mxCreateDoubleMatrix(K + 1, 1, mxREAL); for (size_t k = 0; k <= K; ++k) mxGetPr(pout[1])[k] = (double)off[k]; }
        if (nout > 2) {
            const size_t n = (size_t)off[K];
            if (dil) { pout[2] = mxCreateLogicalMatrix(n, 1); for (size_t i = 0; i < n; ++i) mxGetLogicals(pout[2])[i] = ((uint8_t *)out)[i] != 0; }
            else { pout[2] = mxCreateNumericMatrix(n, 1, mxSINGLE_CLASS, mxREAL); if (n) memcpy(mxGetData(pout[2]), out, n * sizeof(float)); }
        }
        if (nout > 3) { pout[3] = mxCreateLogicalMatrix(K, 1); for (size_t k = 0; k < K; ++k) mxGetLogicals(pout[3])[k] = hc[k] != 0; }
        return;
    }
    if (!strcmp(cmd, "trim_spatial")) {                         // [keep, ind_small, host_col] = cnmfe_mex('trim_spatial', h, A, d1, d2, thr, sz, min_pixel)
        if (nin != 8) FAIL("trim_spatial: 8 inputs required");
        Csc A = csc_of(pin[2]);
        const size_t K = (size_t)A.K;
        uint8_t *keep = (uint8_t *)mxCalloc((size_t)A.nnz + 1, 1), *small = (uint8_t *)mxCalloc(K + 1, 1), *hc = (uint8_t *)mxCalloc(K + 1, 1);
        CHECK(cnmfe_trim_spatial(c, (int32_t)mxGetScalar(pin[3]), (int32_t)mxGetScalar(pin[4]), A.K, A.cp, A.ri, A.v, mxGetScalar(pin[5]), (int32_t)mxGetScalar(pin[6]),
                                 (int32_t)mxGetScalar(pin[7]), keep, small, hc, CNMFE_HOST));
        pout[0] = mxCreateLogicalMatrix((size_t)A.nnz, 1);
        for (int64_t i = 0; i < A.nnz; ++i) mxGetLogicals(pout[0])[i] = keep[i] != 0;
        if (nout > 1) { pout[1] = mxCreateLogicalMatrix(K, 1); for (size_t k = 0; k < K; ++k) mxGetLogicals(pout[1])[k] = small[k] != 0; }
        if (nout > 2) { pout[2] = mxCreateLogicalMatrix(K, 1); for (size_t k = 0; k < K; ++k) mxGetLogicals(pout[2])[k] = hc[k] != 0; }
        return;
    }
    if (!strcmp(cmd, "set_option")) {                           // cnmfe_mex('set_option', h, name, value)
        if (nin != 4) FAIL("set_option: 4 inputs required (h, name, value)");
        char name[48];
        if (!mxIsChar(pin[2]) || mxGetString(pin[2], name, sizeof(name))) FAIL("set_option: bad option name");
        CHECK(cnmfe_set_option(c, name, (int64_t)mxGetScalar(pin[3])));
        return;
    }
    if (!strcmp(cmd, "synchronize")) {
        if (nin != 2) FAIL("synchronize: 2 inputs required");
        CHECK(cnmfe_synchronize(c));
        return;
    }
    if (!strcmp(cmd, "temporal_jobs_sweep")) {                  // the Gauss-Seidel levels of every queued job, one launch per level (update_temporal_parallel.m:112-186 is a parfor)
        if (nin != 2) FAIL("temporal_jobs_sweep: 2 inputs required");
        CHECK(cnmfe_temporal_jobs_sweep(c));
        return;
    }
    if (!strcmp(cmd, "stitch_add_job")) {                       // cnmfe_mex('stitch_add_job', h, job, ind): ind 1-based rows (double or int32)
        if (nin != 4) FAIL("stitch_add_job: 4 inputs required (h, job, ind)");
        const int32_t n = (int32_t)mxGetNumberOfElements(pin[3]);
        int32_t *ind = (int32_t *)mxMalloc(((size_t)n + 1) * sizeof(int32_t));
        if (mxIsInt32(pin[3])) { const int32_t *src = (const int32_t *)mxGetData(pin[3]); for (int32_t i = 0; i < n; ++i) ind[i] = src[i] - 1; }
        else if (mxIsDouble(pin[3])) { const double *src = mxGetPr(pin[3]); for (int32_t i = 0; i < n; ++i) ind[i] = (int32_t)src[i] - 1; }
        else FAIL("stitch_add_job: ind must be double or int32");
        CHECK(cnmfe_stitch_add_job(c, (int32_t)mxGetScalar(pin[2]), n, ind));
        return;
    }
    if (!strcmp(cmd, "stitch_finish_async")) {                  // cnmfe_mex('stitch_finish_async', h, subtract_min, K, T)
        if (nin != 5) FAIL("stitch_finish_async: 5 inputs required (h, subtract_min, K, T)");
        const int hi = (int)mxGetScalar(pin[1]) - 1;
        const size_t K = (size_t)mxGetScalar(pin[3]), T = (size_t)mxGetScalar(pin[4]);
        if (g_stitch[hi].pinned) { cnmfe_host_free(g_stitch[hi].pinned); g_stitch[hi].pinned = NULL; }
        g_stitch[hi].pinned = (float *)cnmfe_host_alloc((K * T + 1) * sizeof(float));
        if (!g_stitch[hi].pinned) FAIL("%s", cnmfe_last_error());
        g_stitch[hi].K = K; g_stitch[hi].T = T;
        CHECK(cnmfe_stitch_finish_async(c, mxGetScalar(pin[2]) != 0, g_stitch[hi].pinned));
        return;
    }
    if (!strcmp(cmd, "stitch_collect")) {                       // C_raw = cnmfe_mex('stitch_collect', h)   (single, K x T)
        if (nin != 2) FAIL("stitch_collect: 2 inputs required");
        const int hi = (int)mxGetScalar(pin[1]) - 1;
        if (!g_stitch[hi].pinned) FAIL("stitch_collect: no stitch_finish_async outstanding on this context");
        CHECK(cnmfe_stitch_wait(c));
        const size_t K = g_stitch[hi].K, T = g_stitch[hi].T;
        pout[0] = mxCreateNumericMatrix(K, T, mxSINGLE_CLASS, mxREAL);
        float *dst = (float *)mxGetData(pout[0]);
        const float *src = g_stitch[hi].pinned;                 // row-major K x T -> MATLAB's column-major
        for (size_t k = 0; k < K; ++k) for (size_t t = 0; t < T; ++t) dst[t * K + k] = src[k * T + t];
        cnmfe_host_free(g_stitch[hi].pinned); g_stitch[hi].pinned = NULL;
        return;
    }
    if (!strcmp(cmd, "spatial_collect")) {                      // A = cnmfe_mex('spatial_collect', h, q)
        if (nin != 3) FAIL("spatial_collect: 3 inputs required (h, q)");
        const int q = (int)mxGetScalar(pin[2]) - 1;
        if (q < 0 || q >= MAX_PEND || !g_pend[q].used || g_pend[q].c != c) FAIL("spatial_collect: no such queued update on this context");
        Pending *P = &g_pend[q];
        const int rc = cnmfe_ticket_wait(c, P->ticket);
        const mxArray *IND = P->ind;
        const size_t K = mxGetN(IND);
        if (rc == 0) {
            pout[0] = mxCreateSparse(mxGetM(IND), K, P->nnz > 0 ? (size_t)P->nnz : 1, mxREAL);           // same pattern as IND
            memcpy(mxGetJc(pout[0]), mxGetJc(IND), (K + 1) * sizeof(mwIndex));
            memcpy(mxGetIr(pout[0]), mxGetIr(IND), (size_t)P->nnz * sizeof(mwIndex));
            for (int64_t i = 0; i < P->nnz; ++i) mxGetPr(pout[0])[i] = P->pinned[i];
        }
        cnmfe_host_free(P->pinned); mxDestroyArray(P->ind); P->pinned = NULL; P->ind = NULL; P->used = 0;
        CHECK(rc);
        return;
    }
    if (nin < 3) FAIL("missing patch id");
    const int pid = (int)mxGetScalar(pin[2]);
    if (!strcmp(cmd, "patch")) {
        if (nin != 8) FAIL("patch: 8 inputs required");
        if (mxGetNumberOfElements(pin[3]) != 4 || mxGetNumberOfElements(pin[4]) != 4) FAIL("patch: positions are [r0 r1 c0 c1]");
        int32_t pr[4], br[4];
        for (int i = 0; i < 4; ++i) { pr[i] = (int32_t)mxGetPr(pin[3])[i]; br[i] = (int32_t)mxGetPr(pin[4])[i]; }
        int slot = 0;
        while (slot < g_ndims && !(g_dims[slot].c == c && g_dims[slot].pid == pid)) ++slot;
        if (slot >= MAX_DIMS) FAIL("patch: this gateway keeps the block sizes of at most %d patches", MAX_DIMS);
        CHECK(cnmfe_patch_create(c, pid, pr, br, (int32_t)mxGetScalar(pin[5]), (int32_t)mxGetScalar(pin[6]), (int64_t)mxGetScalar(pin[7])));
        g_dims[slot].c = c; g_dims[slot].pid = pid; g_dims[slot].nr_b = br[1] - br[0] + 1; g_dims[slot].nc_b = br[3] - br[2] + 1; g_dims[slot].peel_n = 0;
        g_dims[slot].nr_p = pr[1] - pr[0] + 1; g_dims[slot].nc_p = pr[3] - pr[2] + 1; g_dims[slot].T = (int64_t)mxGetScalar(pin[7]); g_dims[slot].peel_nr = g_dims[slot].peel_nc = 0;
        if (slot == g_ndims) ++g_ndims;
    } else if (!strcmp(cmd, "upload")) {
        if (nin != 5) FAIL("upload: 5 inputs required");
        const mxArray *Y = pin[3];
        const int dt = mxIsSingle(Y) ? CNMFE_F32 : mxIsDouble(Y) ? CNMFE_F64 : mxIsUint16(Y) ? CNMFE_U16 : mxIsUint8(Y) ? CNMFE_U8 : -1;
        if (dt < 0) FAIL("upload: unsupported class %s", mxGetClassName(Y));
        CHECK(cnmfe_upload_block(c, pid, mxGetData(Y), dt, CNMFE_HOST, (int64_t)mxGetScalar(pin[4]), (int64_t)mxGetN(Y)));
    } else if (!strcmp(cmd, "ring_init")) {
        if (nin < 4) FAIL("ring_init: radius required");
        CHECK(cnmfe_ring_init(c, pid, (int32_t)mxGetScalar(pin[3]), nin > 4 && !mxIsEmpty(pin[4]) ? (int32_t)mxGetScalar(pin[4]) : 0));
    } else if (!strcmp(cmd, "fit_reserve")) {
        CHECK(cnmfe_fit_reserve(c, pid));
    } else if (!strcmp(cmd, "first_run")) {
        int f = 0;
        CHECK(cnmfe_ring_first_run(c, pid, &f));
        pout[0] = mxCreateLogicalScalar(f != 0);
    } else if (!strcmp(cmd, "fit_ring")) {
        if (nin != 6 && nin != 7) FAIL("fit_ring: 6 or 7 inputs required (h, pid, A, C, with_projection[, thresh_outlier])");
        Csc A = csc_of(pin[3]);
        Traces Cm = traces_of(pin[4], A.K);
        int64_t info[4];
        CHECK(cnmfe_fit_ring_model(c, pid, A.K, A.cp, A.ri, A.v, Cm.ptr, Cm.order, nin > 6 ? mxGetScalar(pin[6]) : mxGetNaN(), mxGetScalar(pin[5]) != 0, NULL, info));
        pout[0] = info_of(info);
    } else if (!strcmp(cmd, "residual")) {
        if (nin != 5) FAIL("residual: 5 inputs required");
        Csc A = csc_of(pin[3]);
        Traces Cm = traces_of(pin[4], A.K);
        CHECK(cnmfe_residual(c, pid, A.K, A.cp, A.ri, A.v, Cm.ptr, Cm.order, NULL, CNMFE_HOST));
    } else if (!strcmp(cmd, "spatial")) {
        if (nin != 9) FAIL("spatial: 9 inputs required");
        char alg[16];
        if (mxGetString(pin[3], alg, sizeof(alg))) FAIL("spatial: bad algorithm name");
        const int a = !strcmp(alg, "hals") ? CNMFE_SPATIAL_HALS : !strcmp(alg, "hals_thresh") ? CNMFE_SPATIAL_HALS_THRESH : !strcmp(alg, "nnls") ? CNMFE_SPATIAL_NNLS : -1;
        if (a < 0) FAIL("spatial: unknown algorithm '%s'", alg);
        if (!mxIsSparse(pin[6])) FAIL("spatial: IND must be sparse");
        Csc A = csc_of(pin[4]), IND = csc_of(pin[6]);
        Traces Cm = traces_of(pin[5], A.K);
        float *sn = mxIsEmpty(pin[7]) ? NULL : f32_of(pin[7], NULL);
        float *out = (float *)mxCalloc((size_t)IND.nnz + 1, sizeof(float));
        CHECK(cnmfe_update_spatial(c, pid, a, A.K, A.cp, A.ri, A.v, Cm.ptr, Cm.order, IND.cp, IND.ri, sn, (int32_t)mxGetScalar(pin[8]), out));
        pout[0] = mxCreateSparse(mxGetM(pin[6]), (size_t)IND.K, (size_t)IND.nnz > 0 ? (size_t)IND.nnz : 1, mxREAL);       // same pattern as IND
        memcpy(mxGetJc(pout[0]), mxGetJc(pin[6]), ((size_t)IND.K + 1) * sizeof(mwIndex));
        memcpy(mxGetIr(pout[0]), mxGetIr(pin[6]), (size_t)IND.nnz * sizeof(mwIndex));
        for (int64_t i = 0; i < IND.nnz; ++i) mxGetPr(pout[0])[i] = out[i];
    } else if (!strcmp(cmd, "temporal")) {
        if (nin != 6) FAIL("temporal: 6 inputs required");
        Csc A = csc_of(pin[3]);
        Traces Cm = traces_of(pin[4], A.K);
        const size_t K = (size_t)A.K, T = mxIsInt32(pin[4]) ? 0 : mxGetN(pin[4]);
        if (nout > 0 && T == 0) FAIL("temporal: outputs need the trace matrix itself (row lists carry no T); use the stitch commands instead");
        float *Co = nout > 0 ? (float *)mxMalloc((K * T + 1) * sizeof(float)) : NULL, *Cr = nout > 1 ? (float *)mxMalloc((K * T + 1) * sizeof(float)) : NULL;
        float *aa = (float *)mxMalloc((K + 1) * sizeof(float));
        CHECK(cnmfe_hals_temporal(c, pid, A.K, A.cp, A.ri, A.v, Cm.ptr, Cm.order, (int32_t)mxGetScalar(pin[5]), Co, Cr, aa));
        if (nout > 0) pout[0] = to_double(Co, K, T);
        if (nout > 1) pout[1] = to_double(Cr, K, T);
        if (nout > 2) pout[2] = to_double(aa, K, 1);
    } else if (!strcmp(cmd, "temporal_job")) {                 // job = cnmfe_mex('temporal_job', h, pid, A_patch, C_or_rows, maxIter)
        if (nin != 6) FAIL("temporal_job: 6 inputs required");
        Csc A = csc_of(pin[3]);
        Traces Cm = traces_of(pin[4], A.K);
        int32_t job = -1;
        CHECK(cnmfe_hals_temporal_job(c, pid, A.K, A.cp, A.ri, A.v, Cm.ptr, Cm.order, (int32_t)mxGetScalar(pin[5]), NULL, NULL, &job));
        pout[0] = mxCreateDoubleScalar((double)job);
    } else if (!strcmp(cmd, "spatial_queue")) {                // q = cnmfe_mex('spatial_queue', h, pid, alg, A_patch, C_or_rows, IND_patch, sn, param)
        if (nin != 9) FAIL("spatial_queue: 9 inputs required");
        char alg[16];
        if (mxGetString(pin[3], alg, sizeof(alg))) FAIL("spatial_queue: bad algorithm name");
        const int a = !strcmp(alg, "hals") ? CNMFE_SPATIAL_HALS : !strcmp(alg, "hals_thresh") ? CNMFE_SPATIAL_HALS_THRESH : !strcmp(alg, "nnls") ? CNMFE_SPATIAL_NNLS : -1;
        if (a < 0) FAIL("spatial_queue: unknown algorithm '%s'", alg);
        if (!mxIsSparse(pin[6])) FAIL("spatial_queue: IND must be sparse");
        int q = 0;
        while (q < MAX_PEND && g_pend[q].used) ++q;
        if (q == MAX_PEND) FAIL("spatial_queue: too many updates queued and not collected");
        Csc A = csc_of(pin[4]), IND = csc_of(pin[6]);
        Traces Cm = traces_of(pin[5], A.K);
        float *sn = mxIsEmpty(pin[7]) ? NULL : f32_of(pin[7], NULL);
        CHECK(cnmfe_update_spatial(c, pid, a, A.K, A.cp, A.ri, A.v, Cm.ptr, Cm.order, IND.cp, IND.ri, sn, (int32_t)mxGetScalar(pin[8]), NULL));   // A_out == NULL: deferred
        Pending *P = &g_pend[q];
        P->pinned = (float *)cnmfe_host_alloc(((size_t)IND.nnz + 1) * sizeof(float));
        if (!P->pinned) FAIL("%s", cnmfe_last_error());
        const int rc = cnmfe_update_spatial_fetch_async(c, P->pinned, IND.nnz, &P->ticket);
        if (rc != 0) { cnmfe_host_free(P->pinned); P->pinned = NULL; CHECK(rc); }
        P->ind = mxDuplicateArray(pin[6]);
        mexMakeArrayPersistent(P->ind);
        P->c = c; P->nnz = IND.nnz; P->used = 1;
        pout[0] = mxCreateDoubleScalar((double)(q + 1));
    } else if (!strcmp(cmd, "temporal_deconv")) {
        if (nin != 9) FAIL("temporal_deconv: 9 inputs required (h, pid, A, C, maxIter, smin, max_tau, pars)");
        Csc A = csc_of(pin[3]);
        const size_t K = (size_t)A.K, T = mxGetN(pin[4]);
        if (mxIsInt32(pin[4])) FAIL("temporal_deconv: pass the trace matrix itself");
        Traces Cm = traces_of(pin[4], A.K);
        cnmfe_deconv_opts o; deconv_opts_of(&o, mxGetScalar(pin[6]), mxGetScalar(pin[7]));
        float *kp = (float *)mxCalloc(K + 1, sizeof(float));
        if (!mxIsEmpty(pin[8])) { size_t n; float *p0 = f32_of(pin[8], &n); if (n != K) FAIL("temporal_deconv: pars must have K entries"); memcpy(kp, p0, K * sizeof(float)); }
        float *Co = nout > 0 ? (float *)mxMalloc((K * T + 1) * sizeof(float)) : NULL, *Cr = nout > 1 ? (float *)mxMalloc((K * T + 1) * sizeof(float)) : NULL;
        float *S = nout > 2 ? (float *)mxMalloc((K * T + 1) * sizeof(float)) : NULL;
        float *sn = (float *)mxMalloc((K + 1) * sizeof(float)), *aa = (float *)mxMalloc((K + 1) * sizeof(float));
        CHECK(cnmfe_hals_temporal_deconv(c, pid, A.K, A.cp, A.ri, A.v, Cm.ptr, Cm.order, (int32_t)mxGetScalar(pin[5]), &o, kp, Co, Cr, S, sn, aa));
        if (nout > 0) pout[0] = to_double(Co, K, T);
        if (nout > 1) pout[1] = to_double(Cr, K, T);
        if (nout > 2) pout[2] = to_double(S, K, T);
        if (nout > 3) pout[3] = to_double(kp, K, 1);
        if (nout > 4) pout[4] = to_double(sn, K, 1);
        if (nout > 5) pout[5] = to_double(aa, K, 1);
    } else if (!strcmp(cmd, "fast_temporal")) {
        if (nin != 5) FAIL("fast_temporal: 5 inputs required (h, pid, A, T)");
        Csc A = csc_of(pin[3]);
        const size_t K = (size_t)A.K, T = (size_t)mxGetScalar(pin[4]);
        float *Cr = nout > 0 ? (float *)mxMalloc((K * T + 1) * sizeof(float)) : NULL, *aa = (float *)mxMalloc((K + 1) * sizeof(float));
        CHECK(cnmfe_fast_temporal(c, pid, A.K, A.cp, A.ri, A.v, CNMFE_COLMAJOR, Cr, aa));
        if (nout > 0) pout[0] = to_double(Cr, K, T);
        if (nout > 1) pout[1] = to_double(aa, K, 1);
    } else if (!strcmp(cmd, "compute_rss")) {
        if (nin != 7) FAIL("compute_rss: 7 inputs required (h, pid, A, C, b0_block, b0_new)");
        Csc A = csc_of(pin[3]);
        Traces Cm = traces_of(pin[4], A.K);
        float *bb = f32_of(pin[5], NULL), *bn = f32_of(pin[6], NULL);
        double rss = 0.0;
        CHECK(cnmfe_compute_rss(c, pid, A.K, A.cp, A.ri, A.v, Cm.ptr, Cm.order, bb, bn, &rss));
        pout[0] = mxCreateDoubleScalar(rss);
    } else if (!strcmp(cmd, "reconstruct_background")) {
        if (nin != 7) FAIL("reconstruct_background: 7 inputs required (h, pid, b0_block, b0_new, frame0, nframes)");
        size_t nb = 0, nn = 0;
        float *bb = f32_of(pin[3], &nb), *bn = f32_of(pin[4], &nn);
        const int64_t f0 = (int64_t)mxGetScalar(pin[5]), nf = (int64_t)mxGetScalar(pin[6]);
        if (nf <= 0) FAIL("reconstruct_background: nframes must be positive");
        pout[0] = mxCreateNumericMatrix(nn, (size_t)nf, mxSINGLE_CLASS, mxREAL);
        CHECK(cnmfe_reconstruct_background(c, pid, bb, bn, f0, nf, (float *)mxGetData(pout[0]), CNMFE_HOST));
    } else if (!strcmp(cmd, "df_add_background")) {            // cnmfe_mex('df_add_background', h, pid, b0_block, b0_new_patch, A_patch, ind): all frames of the patch, after 'residual'
        if (nin != 7) FAIL("df_add_background: 7 inputs required (h, pid, b0_block, b0_new, A_patch, ind)");
        Csc A = csc_of(pin[5]);
        size_t n = 0;
        int32_t *ind = ind_of(pin[6], &n);
        if (n != (size_t)A.K) FAIL("df_add_background: one accumulator row per column of A");
        CHECK(cnmfe_df_add_background(c, pid, f32_of(pin[3], NULL), f32_of(pin[4], NULL), A.K, A.cp, A.ri, A.v, ind));
    } else if (!strcmp(cmd, "df_add_background_ssub")) {       // cnmfe_mex('df_add_background_ssub', h, pid, b0_new_patch, A_patch, ind): after 'background_ssub'
        if (nin != 6) FAIL("df_add_background_ssub: 6 inputs required (h, pid, b0_new, A_patch, ind)");
        Csc A = csc_of(pin[4]);
        size_t n = 0;
        int32_t *ind = ind_of(pin[5], &n);
        if (n != (size_t)A.K) FAIL("df_add_background_ssub: one accumulator row per column of A");
        CHECK(cnmfe_df_add_background_ssub(c, pid, f32_of(pin[3], NULL), A.K, A.cp, A.ri, A.v, ind));
    } else if (!strcmp(cmd, "demix_frames") || !strcmp(cmd, "demix_frames_ssub")) {
        // [raw, bg, signal, denoised, residual, mixed] = cnmfe_mex('demix_frames', h, pid, b0_block, b0_new_patch, A_patch, CC, ind, col, mix_scale, frame0, stride, nframes)
        // ('demix_frames_ssub': without b0_block, after 'background_ssub').  CC: a Ksel x T matrix (uploaded; ind = []) or 'bound' / 'craw' with ind = the 1-based rows
        // of A_patch's columns in the bound matrix; col: Ksel x 3; frame0 0-based.  The panels are d x nframes single, mixed d x (3 nframes) single holding the uint16 values
        const int full = !strcmp(cmd, "demix_frames"), a0 = full ? 4 : 3;
        if (nin != a0 + 9) FAIL("%s: %d inputs required (h, pid, %sb0_new, A_patch, CC, ind, col, mix_scale, frame0, stride, nframes)", cmd, a0 + 9, full ? "b0_block, " : "");
        size_t nd = 0, ni = 0, ncol = 0;
        float *bb = full ? f32_of(pin[3], NULL) : NULL, *bn = f32_of(pin[a0], &nd);
        Csc A = csc_of(pin[a0 + 1]);
        const float *CC = NULL; int src = CNMFE_COLMAJOR; int32_t *ind = NULL;
        if (mxIsChar(pin[a0 + 2])) {
            char nm[16];
            if (mxGetString(pin[a0 + 2], nm, sizeof(nm))) FAIL("%s: bad source name", cmd);
            src = !strcmp(nm, "bound") ? CNMFE_BOUND : !strcmp(nm, "craw") ? CNMFE_RES_CRAW : -1;
            if (src < 0) FAIL("%s: unknown source '%s' (bound, craw)", cmd, nm);
            ind = ind_of(pin[a0 + 3], &ni);
            if (ni != (size_t)A.K) FAIL("%s: one row of the bound matrix per column of A", cmd);
        } else if (A.K) {
            if (mxGetM(pin[a0 + 2]) != (size_t)A.K) FAIL("%s: CC has %d rows for %d footprints", cmd, (int)mxGetM(pin[a0 + 2]), (int)A.K);
            CC = f32_of(pin[a0 + 2], NULL);
        }
        float *col = f32_of(pin[a0 + 4], &ncol);
        if (ncol != 3 * (size_t)A.K) FAIL("%s: col must be %d x 3", cmd, (int)A.K);
        float *colr = (float *)mxMalloc((ncol + 1) * sizeof(float));       // column-major Ksel x 3 -> row-major
        for (size_t k = 0; k < (size_t)A.K; ++k) for (int m = 0; m < 3; ++m) colr[3 * k + m] = col[k + (size_t)m * A.K];
        const double scale = mxGetScalar(pin[a0 + 5]);
        const int64_t f0 = (int64_t)mxGetScalar(pin[a0 + 6]), st = (int64_t)mxGetScalar(pin[a0 + 7]), nf = (int64_t)mxGetScalar(pin[a0 + 8]);
        if (nf < 0 || nf > 65535) FAIL("%s: nframes outside 0 .. 65535", cmd);
        const int no = nout > 0 ? (nout > 6 ? 6 : nout) : 1;
        float *o[5] = {NULL, NULL, NULL, NULL, NULL};
        for (int j = 0; j < 5 && j < no; ++j) { pout[j] = mxCreateNumericMatrix(nd, (size_t)nf, mxSINGLE_CLASS, mxREAL); o[j] = (float *)mxGetData(pout[j]); }
        uint16_t *mix = no > 5 ? (uint16_t *)mxCalloc(3 * nd * (size_t)nf + 1, sizeof(uint16_t)) : NULL;
        if (full) CHECK(cnmfe_demix_frames(c, pid, bb, bn, A.K, A.cp, A.ri, A.v, CC, src, ind, colr, scale, f0, st, nf, o[0], o[1], o[2], o[3], o[4], mix, CNMFE_HOST));
        else CHECK(cnmfe_demix_frames_ssub(c, pid, bn, A.K, A.cp, A.ri, A.v, CC, src, ind, colr, scale, f0, st, nf, o[0], o[1], o[2], o[3], o[4], mix, CNMFE_HOST));
        if (no > 5) {
            pout[5] = mxCreateNumericMatrix(nd, 3 * (size_t)nf, mxSINGLE_CLASS, mxREAL);
            float *p = (float *)mxGetData(pout[5]);
            for (size_t i = 0; i < 3 * nd * (size_t)nf; ++i) p[i] = (float)mix[i];
        }
    } else if (!strcmp(cmd, "init_temporal")) {                // [C, C_raw, AA, S, pars, sn] = cnmfe_mex('init_temporal', h, pid, A_block, iters_plain, iters_last, smin, max_tau)   initTemporal.m:160-168
        if (nin != 6 && nin != 8) FAIL("init_temporal: 6 inputs required, 8 with deconvolution (h, pid, A_block, iters_plain, iters_last[, smin, max_tau])");
        int slot = 0;
        while (slot < g_ndims && !(g_dims[slot].c == c && g_dims[slot].pid == pid)) ++slot;
        if (slot == g_ndims) FAIL("init_temporal: patch %d was not created through this gateway", pid);
        if (!mxIsSparse(pin[3])) FAIL("init_temporal: A_block must be sparse (block rows x K)");
        Csc A = csc_of(pin[3]);
        const size_t K = (size_t)A.K, T = (size_t)g_dims[slot].T;
        const int dec = nin == 8;
        if (!dec && nout > 3) FAIL("init_temporal: S, pars and sn exist with deconvolution only (give smin and max_tau)");
        cnmfe_deconv_opts o;
        if (dec) deconv_opts_of(&o, mxGetScalar(pin[6]), mxGetScalar(pin[7]));
        float *Co = (float *)mxMalloc((K * T + 1) * sizeof(float)), *Cr = nout > 1 ? (float *)mxMalloc((K * T + 1) * sizeof(float)) : NULL;
        float *AA = (float *)mxMalloc((K + 1) * sizeof(float));
        float *S = nout > 3 ? (float *)mxMalloc((K * T + 1) * sizeof(float)) : NULL, *kp = nout > 4 ? (float *)mxMalloc((K + 1) * sizeof(float)) : NULL;
        float *sn = nout > 5 ? (float *)mxMalloc((K + 1) * sizeof(float)) : NULL;
        CHECK(cnmfe_init_temporal(c, pid, A.K, A.cp, A.ri, A.v, (int32_t)mxGetScalar(pin[4]), (int32_t)mxGetScalar(pin[5]), dec ? &o : NULL, Co, Cr, S, kp, sn, AA, CNMFE_COLMAJOR));
        pout[0] = to_double(Co, K, T);
        if (nout > 1) pout[1] = to_double(Cr, K, T);
        if (nout > 2) pout[2] = to_double(AA, K, 1);
        if (nout > 3) pout[3] = to_double(S, K, T);
        if (nout > 4) pout[4] = to_double(kp, K, 1);
        if (nout > 5) pout[5] = to_double(sn, K, 1);
    } else if (!strcmp(cmd, "set_noise")) {                    // cnmfe_mex('set_noise', h, pid, sn_block): read by the outlier branch of the ring fit
        if (nin != 4) FAIL("set_noise: 4 inputs required");
        CHECK(cnmfe_set_noise(c, pid, f32_of(pin[3], NULL)));
    } else if (!strcmp(cmd, "estimate_noise")) {               // sn_block = cnmfe_mex('estimate_noise', h, pid, d_b, nframes)   Sources2D.m:328-379 per pixel
        if (nin != 5) FAIL("estimate_noise: 5 inputs required");
        const size_t db = (size_t)mxGetScalar(pin[3]);
        float *sn = (float *)mxMalloc((db + 1) * sizeof(float));
        CHECK(cnmfe_estimate_noise(c, pid, (int64_t)mxGetScalar(pin[4]), sn));
        pout[0] = to_double(sn, db, 1);
    } else if (!strcmp(cmd, "seed_images")) {                  // [Cn_block, PNR_block] = cnmfe_mex('seed_images', h, pid, psf, nframes, Q)   correlation_image_endoscope.m:36-96
        if (nin != 5 && nin != 6) FAIL("seed_images: 5 or 6 inputs required");
        int slot = 0;
        while (slot < g_ndims && !(g_dims[slot].c == c && g_dims[slot].pid == pid)) ++slot;
        if (slot == g_ndims) FAIL("seed_images: patch %d was not created through this gateway", pid);
        const size_t nrb = (size_t)g_dims[slot].nr_b, ncb = (size_t)g_dims[slot].nc_b;
        const mxArray *F = pin[3];
        if (!mxIsEmpty(F) && mxGetM(F) != mxGetN(F)) FAIL("seed_images: psf must be square");
        const int32_t pn = mxIsEmpty(F) ? 0 : (int32_t)mxGetM(F);
        const float *psf = pn ? f32_of(F, NULL) : NULL;
        const int64_t nf = (int64_t)mxGetScalar(pin[4]);
        const double *Q = NULL; int32_t M = 0;
        if (nin == 6 && !mxIsEmpty(pin[5])) {
            if (!mxIsDouble(pin[5]) || mxIsSparse(pin[5]) || (int64_t)mxGetM(pin[5]) != nf) FAIL("seed_images: Q must be a full double nframes x M matrix");
            Q = mxGetPr(pin[5]); M = (int32_t)mxGetN(pin[5]);
        }
        float *cn = (float *)mxMalloc((nrb * ncb + 1) * sizeof(float)), *pnr = (float *)mxMalloc((nrb * ncb + 1) * sizeof(float));
        CHECK(cnmfe_seed_images(c, pid, psf, pn, 0, nf, Q, M, 3.0f, cn, pnr));
        pout[0] = to_double(cn, nrb, ncb);
        if (nout > 1) pout[1] = to_double(pnr, nrb, ncb);
    } else if (!strcmp(cmd, "seed_images_ds")) {               // [Cn_ds, PNR_ds] = cnmfe_mex('seed_images_ds', h, pid, ssub, tsub, psf, nframes, Q)   correlation_pnr_parallel.m:81-96
        if (nin != 7 && nin != 8) FAIL("seed_images_ds: 7 or 8 inputs required");
        int slot = 0;
        while (slot < g_ndims && !(g_dims[slot].c == c && g_dims[slot].pid == pid)) ++slot;
        if (slot == g_ndims) FAIL("seed_images_ds: patch %d was not created through this gateway", pid);
        const int ssub = (int)mxGetScalar(pin[3]), tsub = (int)mxGetScalar(pin[4]);
        if (ssub < 1 || ssub > 8 || tsub < 1) FAIL("seed_images_ds: ssub = %d (1 .. 8), tsub = %d (>= 1)", ssub, tsub);
        const size_t d1s = ((size_t)g_dims[slot].nr_b + ssub - 1) / ssub, d2s = ((size_t)g_dims[slot].nc_b + ssub - 1) / ssub;
        const mxArray *F = pin[5];
        if (!mxIsEmpty(F) && mxGetM(F) != mxGetN(F)) FAIL("seed_images_ds: psf must be square");
        const int32_t pn = mxIsEmpty(F) ? 0 : (int32_t)mxGetM(F);
        const float *psf = pn ? f32_of(F, NULL) : NULL;
        const int64_t nf = (int64_t)mxGetScalar(pin[6]);
        const double *Q = NULL; int32_t M = 0;
        if (nin == 8 && !mxIsEmpty(pin[7])) {
            if (!mxIsDouble(pin[7]) || mxIsSparse(pin[7]) || (int64_t)mxGetM(pin[7]) != nf / tsub) FAIL("seed_images_ds: Q must be a full double floor(nframes / tsub) x M matrix");
            Q = mxGetPr(pin[7]); M = (int32_t)mxGetN(pin[7]);
        }
        float *cn = (float *)mxMalloc((d1s * d2s + 1) * sizeof(float)), *pnr = (float *)mxMalloc((d1s * d2s + 1) * sizeof(float));
        CHECK(cnmfe_seed_images_ds(c, pid, ssub, tsub, psf, pn, nf, Q, M, 3.0f, cn, pnr));
        pout[0] = to_double(cn, d1s, d2s);
        if (nout > 1) pout[1] = to_double(pnr, d1s, d2s);
    } else if (!strcmp(cmd, "peel_open") || !strcmp(cmd, "peel_open_ds") || !strcmp(cmd, "peel_open_residual") || !strcmp(cmd, "peel_open_residual_ds") || !strcmp(cmd, "peel_extract") || !strcmp(cmd, "peel_apply") || !strcmp(cmd, "peel_close")) {
        int slot = 0;
        while (slot < g_ndims && !(g_dims[slot].c == c && g_dims[slot].pid == pid)) ++slot;
        if (slot == g_ndims) FAIL("%s: patch %d was not created through this gateway", cmd, pid);
        int nrb = g_dims[slot].nr_b, ncb = g_dims[slot].nc_b;
        if (!strcmp(cmd, "peel_open_residual")) {              // [Cn_patch, PNR_patch, Sn_patch, Yres] = cnmfe_mex('peel_open_residual', h, pid, A_patch, C_or_rows, psf)
            if (nin != 6) FAIL("peel_open_residual: 6 inputs required");
            const mxArray *F = pin[5];
            if (!mxIsEmpty(F) && mxGetM(F) != mxGetN(F)) FAIL("peel_open_residual: psf must be square");
            const int32_t pn = mxIsEmpty(F) ? 0 : (int32_t)mxGetM(F);
            const float *psf = pn ? f32_of(F, NULL) : NULL;
            Csc A = csc_of(pin[3]);
            Traces Cm = traces_of(pin[4], A.K);
            const size_t nrp = (size_t)g_dims[slot].nr_p, ncp = (size_t)g_dims[slot].nc_p, dp = nrp * ncp;
            float *cn = (float *)mxMalloc((dp + 1) * sizeof(float)), *pnr = (float *)mxMalloc((dp + 1) * sizeof(float)), *sn = (float *)mxMalloc((dp + 1) * sizeof(float));
            mxArray *yres = nout > 3 ? mxCreateNumericMatrix(dp, (size_t)g_dims[slot].T, mxSINGLE_CLASS, mxREAL) : NULL;
            CHECK(cnmfe_peel_open_residual(c, pid, A.K, A.cp, A.ri, A.v, Cm.ptr, Cm.order, psf, pn, 3.0f, cn, pnr, sn, yres ? (float *)mxGetData(yres) : NULL, CNMFE_HOST));
            g_dims[slot].peel_n = g_dims[slot].T; g_dims[slot].peel_nr = (int32_t)nrp; g_dims[slot].peel_nc = (int32_t)ncp;
            pout[0] = to_double(cn, nrp, ncp);
            if (nout > 1) pout[1] = to_double(pnr, nrp, ncp);
            if (nout > 2) pout[2] = to_double(sn, nrp, ncp);
            if (nout > 3) pout[3] = yres;
        } else if (!strcmp(cmd, "peel_open_residual_ds")) {           // [Cn_ds, PNR_ds, Sn_ds, Yds] = cnmfe_mex('peel_open_residual_ds', h, pid, ssub, tsub, A_patch, C_or_rows, psf)
            if (nin != 8) FAIL("peel_open_residual_ds: 8 inputs required");
            const int ssub = (int)mxGetScalar(pin[3]), tsub = (int)mxGetScalar(pin[4]);
            if (ssub < 1 || ssub > 8 || tsub < 1) FAIL("peel_open_residual_ds: ssub = %d (1 .. 8), tsub = %d (>= 1)", ssub, tsub);
            const mxArray *F = pin[7];
            if (!mxIsEmpty(F) && mxGetM(F) != mxGetN(F)) FAIL("peel_open_residual_ds: psf must be square");
            const int32_t pn = mxIsEmpty(F) ? 0 : (int32_t)mxGetM(F);
            const float *psf = pn ? f32_of(F, NULL) : NULL;
            Csc A = csc_of(pin[5]);
            Traces Cm = traces_of(pin[6], A.K);
            const size_t d1s = ((size_t)g_dims[slot].nr_p + ssub - 1) / ssub, d2s = ((size_t)g_dims[slot].nc_p + ssub - 1) / ssub, ds = d1s * d2s;
            const int64_t Ts = g_dims[slot].T / tsub;
            float *cn = (float *)mxMalloc((ds + 1) * sizeof(float)), *pnr = (float *)mxMalloc((ds + 1) * sizeof(float)), *sn = (float *)mxMalloc((ds + 1) * sizeof(float));
            mxArray *yds = nout > 3 ? mxCreateNumericMatrix(ds, (size_t)Ts, mxSINGLE_CLASS, mxREAL) : NULL;
            CHECK(cnmfe_peel_open_residual_ds(c, pid, ssub, tsub, A.K, A.cp, A.ri, A.v, Cm.ptr, Cm.order, psf, pn, 3.0f, cn, pnr, sn, yds ? (float *)mxGetData(yds) : NULL, CNMFE_HOST));
            g_dims[slot].peel_n = Ts; g_dims[slot].peel_nr = (int32_t)d1s; g_dims[slot].peel_nc = (int32_t)d2s;
            pout[0] = to_double(cn, d1s, d2s);
            if (nout > 1) pout[1] = to_double(pnr, d1s, d2s);
            if (nout > 2) pout[2] = to_double(sn, d1s, d2s);
            if (nout > 3) pout[3] = yds;
        } else if (!strcmp(cmd, "peel_open")) {                       // [Cn_block, PNR_block, Sn_block] = cnmfe_mex('peel_open', h, pid, psf, nframes, Q)
            if (nin != 5 && nin != 6) FAIL("peel_open: 5 or 6 inputs required");
            const mxArray *F = pin[3];
            if (!mxIsEmpty(F) && mxGetM(F) != mxGetN(F)) FAIL("peel_open: psf must be square");
            const int32_t pn = mxIsEmpty(F) ? 0 : (int32_t)mxGetM(F);
            const float *psf = pn ? f32_of(F, NULL) : NULL;
            const int64_t nf = (int64_t)mxGetScalar(pin[4]);
            const double *Q = NULL; int32_t M = 0;
            if (nin == 6 && !mxIsEmpty(pin[5])) {
                if (!mxIsDouble(pin[5]) || mxIsSparse(pin[5]) || (int64_t)mxGetM(pin[5]) != nf) FAIL("peel_open: Q must be a full double nframes x M matrix");
                Q = mxGetPr(pin[5]); M = (int32_t)mxGetN(pin[5]);
            }
            const size_t db = (size_t)nrb * (size_t)ncb;
            float *cn = (float *)mxMalloc((db + 1) * sizeof(float)), *pnr = (float *)mxMalloc((db + 1) * sizeof(float)), *sn = (float *)mxMalloc((db + 1) * sizeof(float));
            CHECK(cnmfe_peel_open(c, pid, psf, pn, 0, nf, Q, M, 3.0f, cn, pnr, sn));
            g_dims[slot].peel_n = nf; g_dims[slot].peel_nr = nrb; g_dims[slot].peel_nc = ncb;
            pout[0] = to_double(cn, (size_t)nrb, (size_t)ncb);
            if (nout > 1) pout[1] = to_double(pnr, (size_t)nrb, (size_t)ncb);
            if (nout > 2) pout[2] = to_double(sn, (size_t)nrb, (size_t)ncb);
        } else if (!strcmp(cmd, "peel_open_ds")) {                    // [Cn_ds, PNR_ds, Sn_ds, Yds] = cnmfe_mex('peel_open_ds', h, pid, ssub, tsub, psf, nframes, Qpre)
            if (nin != 7 && nin != 8) FAIL("peel_open_ds: 7 or 8 inputs required");
            const int ssub = (int)mxGetScalar(pin[3]), tsub = (int)mxGetScalar(pin[4]);
            if (ssub < 1 || ssub > 8 || tsub < 1) FAIL("peel_open_ds: ssub = %d (1 .. 8), tsub = %d (>= 1)", ssub, tsub);
            const size_t d1s = ((size_t)nrb + ssub - 1) / ssub, d2s = ((size_t)ncb + ssub - 1) / ssub, ds = d1s * d2s;
            const mxArray *F = pin[5];
            if (!mxIsEmpty(F) && mxGetM(F) != mxGetN(F)) FAIL("peel_open_ds: psf must be square");
            const int32_t pn = mxIsEmpty(F) ? 0 : (int32_t)mxGetM(F);
            const float *psf = pn ? f32_of(F, NULL) : NULL;
            const int64_t nf = (int64_t)mxGetScalar(pin[6]);
            if (nf < 1 || nf > g_dims[slot].T) FAIL("peel_open_ds: nframes = %lld of %lld", (long long)nf, (long long)g_dims[slot].T);
            const int64_t Ts = nf / tsub;
            const double *Q = NULL; int32_t M = 0;
            if (nin == 8 && !mxIsEmpty(pin[7])) {
                if (!mxIsDouble(pin[7]) || mxIsSparse(pin[7]) || (int64_t)mxGetM(pin[7]) != nf) FAIL("peel_open_ds: Qpre must be a full double nframes x M matrix (the FULL-LENGTH basis)");
                Q = mxGetPr(pin[7]); M = (int32_t)mxGetN(pin[7]);
            }
            float *cn = (float *)mxMalloc((ds + 1) * sizeof(float)), *pnr = (float *)mxMalloc((ds + 1) * sizeof(float)), *sn = (float *)mxMalloc((ds + 1) * sizeof(float));
            mxArray *yds = nout > 3 ? mxCreateNumericMatrix(ds, (size_t)Ts, mxSINGLE_CLASS, mxREAL) : NULL;
            CHECK(cnmfe_peel_open_ds(c, pid, ssub, tsub, psf, pn, nf, Q, M, 3.0f, cn, pnr, sn, yds ? (float *)mxGetData(yds) : NULL, CNMFE_HOST));
            g_dims[slot].peel_n = Ts; g_dims[slot].peel_nr = (int32_t)d1s; g_dims[slot].peel_nc = (int32_t)d2s;
            pout[0] = to_double(cn, d1s, d2s);
            if (nout > 1) pout[1] = to_double(pnr, d1s, d2s);
            if (nout > 2) pout[2] = to_double(sn, d1s, d2s);
            if (nout > 3) pout[3] = yds;
        } else if (!strcmp(cmd, "peel_close")) {               // cnmfe_mex('peel_close', h, pid)
            if (nin != 3) FAIL("peel_close: 3 inputs required");
            CHECK(cnmfe_peel_close(c, pid));
            g_dims[slot].peel_n = 0;
        } else {
            if (nin < 6) FAIL("%s: the seed (r, c) and gSiz are required", cmd);
            const int r = (int)mxGetScalar(pin[3]) - 1, cc = (int)mxGetScalar(pin[4]) - 1, g = (int)mxGetScalar(pin[5]);
            const int64_t nf = g_dims[slot].peel_n;
            if (nf <= 0) FAIL("%s: patch %d has no open peel session ('peel_open')", cmd, pid);
            nrb = g_dims[slot].peel_nr; ncb = g_dims[slot].peel_nc;          // the session's geometry: the block, or the patch of a residual session
            if (r < 0 || r >= nrb || cc < 0 || cc >= ncb || g < 1) FAIL("%s: the seed (%d, %d) lies outside the %d x %d session, or gSiz = %d", cmd, r + 1, cc + 1, nrb, ncb, g);
#define PEEL_LO(x, reach) ((x) - (reach) < 0 ? 0 : (x) - (reach))
#define PEEL_HI(x, reach, n) ((x) + (reach) > (n) - 1 ? (n) - 1 : (x) + (reach))
            const size_t nr1 = (size_t)(PEEL_HI(r, g, nrb) - PEEL_LO(r, g) + 1), nc1 = (size_t)(PEEL_HI(cc, g, ncb) - PEEL_LO(cc, g) + 1);
            const size_t nr2 = (size_t)(PEEL_HI(r, 2 * g, nrb) - PEEL_LO(r, 2 * g) + 1), nc2 = (size_t)(PEEL_HI(cc, 2 * g, ncb) - PEEL_LO(cc, 2 * g) + 1);
            if (!strcmp(cmd, "peel_extract")) {                // [corr, ai, ci, stats] = cnmfe_mex('peel_extract', h, pid, r, c, gSiz)   extract_ac.m:19-58
                if (nin != 6) FAIL("peel_extract: 6 inputs required");
                mxArray *corr = mxCreateDoubleMatrix(nr1, nc1, mxREAL), *ai = mxCreateDoubleMatrix(nr1, nc1, mxREAL);
                mxArray *ci = mxCreateDoubleMatrix(1, (size_t)nf, mxREAL), *st = mxCreateDoubleMatrix(1, 6, mxREAL);
                CHECK(cnmfe_peel_extract(c, pid, r, cc, g, mxGetPr(corr), mxGetPr(ai), mxGetPr(ci), mxGetPr(st)));
                pout[0] = corr;
                if (nout > 1) pout[1] = ai; else mxDestroyArray(ai);
                if (nout > 2) pout[2] = ci; else mxDestroyArray(ci);
                if (nout > 3) pout[3] = st; else mxDestroyArray(st);
            } else {                                           // [PNR_box2, Cn_box2] = cnmfe_mex('peel_apply', h, pid, r, c, gSiz, ai, Hai, ci, sig, min_pnr, min_corr)
                if (nin != 12) FAIL("peel_apply: 12 inputs required");
                for (int k = 6; k < 9; ++k) if (!mxIsDouble(pin[k]) || mxIsSparse(pin[k])) FAIL("peel_apply: ai, Hai and ci must be full double arrays");
                if (mxGetNumberOfElements(pin[6]) != nr1 * nc1 || mxGetNumberOfElements(pin[7]) != nr2 * nc2 || (int64_t)mxGetNumberOfElements(pin[8]) != nf)
                    FAIL("peel_apply: ai must have %d, Hai %d and ci %d elements", (int)(nr1 * nc1), (int)(nr2 * nc2), (int)nf);
                float *pnr = (float *)mxMalloc((nr2 * nc2 + 1) * sizeof(float)), *cn = (float *)mxMalloc((nr2 * nc2 + 1) * sizeof(float));
                CHECK(cnmfe_peel_apply(c, pid, r, cc, g, mxGetPr(pin[6]), mxGetPr(pin[7]), mxGetPr(pin[8]), mxGetScalar(pin[9]), mxGetScalar(pin[10]), mxGetScalar(pin[11]), pnr, cn));
                pout[0] = to_double(pnr, nr2, nc2);
                if (nout > 1) pout[1] = to_double(cn, nr2, nc2);
            }
#undef PEEL_LO
#undef PEEL_HI
        }
    } else if (!strcmp(cmd, "background_ssub")) {              // cnmfe_mex('background_ssub', h, pid, fit_pid, bg_ssub, A_prev_block, C_or_rows, b0_block)
        if (nin != 8) FAIL("background_ssub: 8 inputs required");
        Csc A = csc_of(pin[5]);
        Traces Cm = traces_of(pin[6], A.K);
        CHECK(cnmfe_background_ssub(c, pid, (int)mxGetScalar(pin[3]), (int32_t)mxGetScalar(pin[4]), A.K, A.cp, A.ri, A.v, Cm.ptr, Cm.order, f32_of(pin[7], NULL)));
    } else if (!strcmp(cmd, "compute_rss_ssub")) {             // rss = cnmfe_mex('compute_rss_ssub', h, pid, A_patch, C_or_rows, b0_new_patch)
        if (nin != 6) FAIL("compute_rss_ssub: 6 inputs required");
        Csc A = csc_of(pin[3]);
        Traces Cm = traces_of(pin[4], A.K);
        double rss = 0.0;
        CHECK(cnmfe_compute_rss_ssub(c, pid, A.K, A.cp, A.ri, A.v, Cm.ptr, Cm.order, f32_of(pin[5], NULL), &rss));
        pout[0] = mxCreateDoubleScalar(rss);
    } else if (!strcmp(cmd, "reconstruct_background_ssub")) {  // Ybg = cnmfe_mex('reconstruct_background_ssub', h, pid, b0_new_patch, frame0, nframes)
        if (nin != 6) FAIL("reconstruct_background_ssub: 6 inputs required");
        size_t nn = 0;
        float *bn = f32_of(pin[3], &nn);
        const int64_t f0 = (int64_t)mxGetScalar(pin[4]), nf = (int64_t)mxGetScalar(pin[5]);
        if (nf <= 0) FAIL("reconstruct_background_ssub: nframes must be positive");
        pout[0] = mxCreateNumericMatrix(nn, (size_t)nf, mxSINGLE_CLASS, mxREAL);
        CHECK(cnmfe_reconstruct_background_ssub(c, pid, bn, f0, nf, (float *)mxGetData(pout[0]), CNMFE_HOST));
    } else if (!strcmp(cmd, "get_sn")) {
        if (nin != 4) FAIL("get_sn: 4 inputs required");
        const size_t d = (size_t)mxGetScalar(pin[3]);
        float *sn = (float *)mxMalloc((d + 1) * sizeof(float));
        CHECK(cnmfe_get_sn(c, pid, sn));
        pout[0] = to_double(sn, d, 1);
    } else if (!strcmp(cmd, "derive")) {
        if (nin != 6) FAIL("derive: 6 inputs required");
        char md[16];
        if (mxGetString(pin[5], md, sizeof(md))) FAIL("derive: bad mode");
        CHECK(cnmfe_patch_derive(c, pid, (int)mxGetScalar(pin[3]), (int32_t)mxGetScalar(pin[4]), !strcmp(md, "nearest") ? CNMFE_DERIVE_NEAREST : CNMFE_DERIVE_BICUBIC));
    } else if (!strcmp(cmd, "fit_ring_ssub")) {
        if (nin != 9 && nin != 10) FAIL("fit_ring_ssub: 9 or 10 inputs required");
        Csc A = csc_of(pin[6]);
        Traces Cm = traces_of(pin[7], A.K);
        int64_t info[4];
        CHECK(cnmfe_fit_ring_model_ssub(c, pid, (int)mxGetScalar(pin[3]), (int)mxGetScalar(pin[4]), (int32_t)mxGetScalar(pin[5]), A.K, A.cp, A.ri, A.v,
                                        Cm.ptr, Cm.order, nin > 9 ? mxGetScalar(pin[9]) : mxGetNaN(), mxGetScalar(pin[8]) != 0, info));
        pout[0] = info_of(info);
    } else if (!strcmp(cmd, "residual_ssub")) {
        if (nin != 7) FAIL("residual_ssub: 7 inputs required");
        Csc A = csc_of(pin[5]);
        Traces Cm = traces_of(pin[6], A.K);
        CHECK(cnmfe_residual_ssub(c, pid, (int)mxGetScalar(pin[3]), (int32_t)mxGetScalar(pin[4]), A.K, A.cp, A.ri, A.v, Cm.ptr, Cm.order, NULL, CNMFE_HOST));
    } else if (!strcmp(cmd, "get_ring")) {
        if (nin != 5) FAIL("get_ring: 5 inputs required (h, pid, d, d_b)");
        int64_t nnz; int32_t p;
        CHECK(cnmfe_ring_nnz(c, pid, &nnz, &p));
        const size_t d = (size_t)mxGetScalar(pin[3]), d_b = (size_t)mxGetScalar(pin[4]);
        int64_t *rp = (int64_t *)mxMalloc((d + 1) * sizeof(int64_t));
        int32_t *col = (int32_t *)mxMalloc(((size_t)nnz + 1) * sizeof(int32_t));
        float *val = (float *)mxMalloc(((size_t)nnz + 1) * sizeof(float)), *b0 = (float *)mxMalloc((d + 1) * sizeof(float));
        CHECK(cnmfe_ring_get_csr(c, pid, rp, col, val));
        CHECK(cnmfe_b0_get(c, pid, b0));
        // CSR (d x d_b) == CSC of the transpose: W' (d_b x d) directly, the caller transposes
        pout[0] = mxCreateSparse(d_b, d, (size_t)nnz > 0 ? (size_t)nnz : 1, mxREAL);
        for (size_t i = 0; i <= d; ++i) mxGetJc(pout[0])[i] = (mwIndex)rp[i];
        for (int64_t e = 0; e < nnz; ++e) { mxGetIr(pout[0])[e] = (mwIndex)col[e]; mxGetPr(pout[0])[e] = val[e]; }
        if (nout > 1) pout[1] = to_double(b0, d, 1);
    } else if (!strcmp(cmd, "set_ring")) {                      // Wt = W{m}.' with the ring's own pattern (what get_ring returned)
        if (nin != 5) FAIL("set_ring: 5 inputs required (h, pid, Wt, b0)");
        int64_t nnz; int32_t p;
        CHECK(cnmfe_ring_nnz(c, pid, &nnz, &p));
        if (!mxIsSparse(pin[3]) || (int64_t)mxGetJc(pin[3])[mxGetN(pin[3])] != nnz) FAIL("set_ring: Wt must be sparse with the ring's %lld entries", (long long)nnz);
        float *val = (float *)mxMalloc(((size_t)nnz + 1) * sizeof(float));
        const double *pr = mxGetPr(pin[3]);
        for (int64_t e = 0; e < nnz; ++e) val[e] = (float)pr[e];
        CHECK(cnmfe_ring_set_values(c, pid, val));
        float *b0 = f32_of(pin[4], NULL);
        CHECK(cnmfe_b0_set(c, pid, b0));
    } else FAIL("unknown command '%s'", cmd);
}
