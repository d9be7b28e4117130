/*
 * cnmfe.h -- C ABI of the MI355X-native CNMF-E factor-update engine.
 *
 * This is the drop-in boundary for ONE path of zhoupc/CNMF_E: the alternating
 * ring-background -> spatial -> temporal update that
 * demos/demo_large_data_1p.m:199-201 runs through
 *   @Sources2D/update_background_parallel.m, update_spatial_parallel.m,
 *   update_temporal_parallel.m
 * and, per patch, through the plain MATLAB functions listed beside each entry
 * point below (file:line are into the reference tree).  A MEX gateway
 * (matlab/cnmfe_mex.cpp) or any FFI (ctypes: cnmf_e_amd/_lib.py) binds exactly
 * these symbols.  No C++/torch types cross the boundary.
 *
 * Conventions
 *   - every call returns 0 on success or a negative CNMFE_E* code;
 *     cnmfe_last_error() returns a thread-local message.  Nothing throws.
 *   - arrays are MATLAB-shaped: the video block is d_b x T column-major, i.e.
 *     frame after frame, each frame an nr_b x nc_b image with the ROW index
 *     fastest.  Pixel linear indices are 0-based inside the ABI.
 *   - sparse matrices are CSC (MATLAB's native layout: Jc = colptr, Ir = rowidx),
 *     64-bit column pointers, 32-bit 0-based row indices, rows sorted per column.
 *   - bulk values are float32 (the engine computes in fp32 with fp64 where it
 *     matters: means, the ring regression Gram/solve, NNLS); index arrays int32/int64.
 *   - the caller owns every pointer it passes; the context owns all device memory.
 *     "out" buffers are caller-allocated; a NULL out pointer means "keep the
 *     result resident only".
 *   - a context is single-threaded and bound to one GPU (one context per GPU,
 *     one process per GPU).
 */
#ifndef CNMFE_H
#define CNMFE_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct cnmfe_ctx cnmfe_ctx;

enum { CNMFE_OK = 0, CNMFE_EINVAL = -1, CNMFE_ENOMEM = -2, CNMFE_EHIP = -3,
       CNMFE_ESTATE = -4, CNMFE_EUNSUPPORTED = -5 };

/* element type of the video handed to cnmfe_upload_block */
enum { CNMFE_F32 = 0, CNMFE_F64 = 1, CNMFE_U16 = 2, CNMFE_U8 = 3, CNMFE_F16 = 4 };
/* where a bulk pointer lives */
enum { CNMFE_HOST = 0, CNMFE_DEVICE = 1 };
/* memory order of a K x T trace matrix */
enum { CNMFE_COLMAJOR = 0 /* MATLAB: element (k,t) at k + t*K */,
       CNMFE_ROWMAJOR = 1 /* numpy:  element (k,t) at k*T + t */,
       CNMFE_BOUND = 2,   /* the pointer is ignored: use the matrix bound with cnmfe_traces_bind */
       CNMFE_BOUND_ROWS = 3 /* the pointer is (const int32_t *) K ascending-or-not 0-based row indices into the bound matrix */ };

/* Bind a K x T trace matrix to the context: one host-to-device transfer, after which every entry point that takes
 * (C, c_order) accepts (NULL, CNMFE_BOUND) for that same matrix (K and T must match) and copies it on the device.
 * obj.C is the same K x T matrix for the background fit, both residual sweeps and the temporal HALS of one iteration
 * (update_background_parallel.m:130, update_temporal_parallel.m:86,91): bind it once, upload it once.  Trace OUTPUTS of a call made
 * with CNMFE_BOUND use the layout the matrix was bound with.  K = 0 unbinds.  A call that works on a SUBSET of the neurons (a patch's
 * C(ind,:), update_*_parallel.m) passes ((const float *)ind, CNMFE_BOUND_ROWS): the rows are gathered on the device, nothing crosses
 * PCIe.  C may be a host or a device pointer (row-major device matrices bind with a device-to-device copy). */
int cnmfe_traces_bind(cnmfe_ctx *ctx, int32_t K, int64_t T, const float *C, int c_order);
/* spatial algorithm (options.spatial_algorithm, CNMFSetParms.m:117) */
enum { CNMFE_SPATIAL_HALS = 0, CNMFE_SPATIAL_HALS_THRESH = 1, CNMFE_SPATIAL_NNLS = 2 };

const char *cnmfe_last_error(void);
const char *cnmfe_version(void);

/* ---- context ------------------------------------------------------------ */
cnmfe_ctx *cnmfe_create(int device);          /* NULL on failure (see cnmfe_last_error) */
void       cnmfe_destroy(cnmfe_ctx *ctx);

/* ---- data plane: one resident block per patch ----------------------------
 * Replaces get_patch_data(mat_data, tmp_patch, frame_range, true)
 * (endoscope/get_patch_data.m:50-93) at update_background_parallel.m:208,
 * update_spatial_parallel.m:147, update_temporal_parallel.m:137: the block is
 * uploaded once and stays in HBM.
 * patch_rect/block_rect = [r0 r1 c0 c1], 1-based inclusive, exactly
 * mat_data.patch_pos{m} / block_pos{m} (distribute_data.m:165-171). */
int cnmfe_patch_create(cnmfe_ctx *ctx, int patch_id, const int32_t patch_rect[4],
                       const int32_t block_rect[4], int32_t d1, int32_t d2, int64_t T);
/* frames [t0, t0+nt) of the block, nt x d_b elements of `dtype`, frame-major */
int cnmfe_upload_block(cnmfe_ctx *ctx, int patch_id, const void *Y, int dtype, int memspace,
                       int64_t t0, int64_t nt);
/* P.Ymean{m} (initComponents_parallel.m:338-339): temporal mean of the BLOCK, d_b doubles */
int cnmfe_get_ymean(cnmfe_ctx *ctx, int patch_id, double *ymean_block);

/* ---- B0: ring pattern -----------------------------------------------------
 * get_nhood(radius, num_neighbors) (endoscope/get_nhood.m:1-25) + the W builder
 * at initComponents_parallel.m:213-236: fixed ring sparsity pattern, W = 1/count,
 * b0 = 0.  num_neighbors <= 0 means [] (all ring pixels). */
int cnmfe_ring_init(cnmfe_ctx *ctx, int patch_id, int32_t radius, int32_t num_neighbors);
int cnmfe_ring_nnz(cnmfe_ctx *ctx, int patch_id, int64_t *nnz, int32_t *p);
/* W{m} as CSR (d x d_b): rowptr[d+1], col[nnz] (block pixel, ascending), val[nnz] */
int cnmfe_ring_get_csr(cnmfe_ctx *ctx, int patch_id, int64_t *rowptr, int32_t *col, float *val);
int cnmfe_ring_set_values(cnmfe_ctx *ctx, int patch_id, const float *val /* nnz, CSR order */);
/* the reference's first-run test, by VALUE inspection of row 1 of W{m}:
 * length(unique(W_old(1,:)))==2   (fit_ring_model.m:25, update_background_parallel.m:143) */
int cnmfe_ring_first_run(cnmfe_ctx *ctx, int patch_id, int *first_run);
int cnmfe_b0_get(cnmfe_ctx *ctx, int patch_id, float *b0 /* d */);
int cnmfe_b0_set(cnmfe_ctx *ctx, int patch_id, const float *b0 /* d */);

/* ---- B1/B2: [W, b0] = fit_ring_model(Y, A, C, W_old, thresh_outlier, sn, ind_patch, with_projection)
 * endoscope/fit_ring_model.m:1-127.  Y = the resident block, W_old = the resident W{m}
 * (first-run detection by value inspection of row 1, :25; ind_active, :28; frame stride k,
 * :60,84-87).  A is d_b x K CSC (block rows), C is K x T.  thresh_outlier = NaN is what every demo runs.  A finite value takes the
 * outlier branch (:50-56: entries of the patch rows above W_old*Bf + thresh_outlier*sn are replaced by W_old*Bf; :62-67: only the frames
 * with at most the nmax/T quantile of outliers are regressed on) -- it needs the noise levels of the block (cnmfe_set_noise, else
 * CNMFE_ESTATE) and computes the Gram of the clipped residual directly (the kept video table does not apply); info[1] is 1 then.
 * info[0]=first_run, info[1]=frame stride k, info[2]=#active pixels (-1 when the call returns without waiting for the device -- b0_out ==
 * NULL on a later run), info[3]=pmax.  Nothing about W_old is asked of the device at call time: pmax and row 1 were copied to pinned memory
 * behind the call that wrote W, so a fit does not drain the stream before it queues its kernels.
 * With b0_out == NULL the call returns while the Gram / solve kernels are still running on the context's stream; every later
 * call on this context is ordered behind them and reports their errors.
 * The first fit of a patch (and the first one after its frame stride k changes) also builds the block-pair covariance table of the
 * resident VIDEO and keeps it with the patch (fp64, 58 bytes per block pixel and needed neighbour pair: 3.8 GB for 512 x 512,
 * radius 15) until the next cnmfe_upload_block; later fits only add the footprint corrections (option "gram_incremental", default 1;
 * 0 = the Gram of Y - A*C from scratch every call).  Results are the same regression either way. */
int cnmfe_fit_ring_model(cnmfe_ctx *ctx, int patch_id, int32_t K, const int64_t *A_colptr,
                         const int32_t *A_rowidx, const float *A_val, const float *C, int c_order,
                         double thresh_outlier, int with_projection,
                         float *b0_out /* d or NULL */, int64_t info[4]);

/* Diagnostics of the last fit's ring solve when it ran out of the cached inverses (option solve_inv, ring_solve_inv.hpp; replaces nothing in the reference --
 * fit_ring_model.m:106 solves every pixel from scratch): out[0] pixels the fast path left to the factorising kernel (more than 8 neurons around the ring, a
 * ridge series that did not converge), out[3] those among them whose inverse was rebuilt; with solve_probe bit 512 also out[1] ridge-series terms taken over
 * all pixels, out[2] pixels that took at least one.  All -1 when the patch has no inverses.  Synchronises the context's stream. */
int cnmfe_ring_solve_stats(cnmfe_ctx *ctx, int patch_id, int64_t out[4]);

/* Optional, once per patch that will be FITTED (after cnmfe_ring_init; with bg_ssub > 1 that is the low-resolution fit patch): allocate the ring fit's large
 * device buffers now -- the block-pair covariance tables, the tiled residual, the window projection's partial sums (18 GB for 512 x 512 x 10000, radius 15) --
 * so that the first cnmfe_fit_ring_model queues its kernels without a hipMalloc in between.  Sizes follow the geometry only; nothing is computed.  The host
 * mirror calls it while it sets the patches up (initComponents_parallel.m:213-236 is where the reference allocates W, b0); a host that does not simply gets
 * the allocations inside its first fit. */
int cnmfe_fit_reserve(cnmfe_ctx *ctx, int patch_id);

/* P.sn: sn = estimate_noise(obj, frame_range, 'psd')  (@Sources2D/Sources2D.m:328-379 -> OASIS_matlab/functions/GetSn.m:19-46) for the block
 * pixels of a patch: the Welch estimate of the first `nframes` frames (the reference's default is min(T, 3000)) of the resident RAW video
 * (pixel mean included, as pwelch sees it).  The per-storage-block bookkeeping of :361-375 (row / column end-1 of every block but the
 * last is dropped) is index arithmetic on the assembled image and stays with the host (sources2d.estimate_noise_image). */
int cnmfe_estimate_noise(cnmfe_ctx *ctx, int patch_id, int64_t nframes, float *sn_block_out /* d_b */);

/* ---- (f) seed images: [Cn, PNR] = correlation_image_endoscope(Ypatch, options) of the block of one patch
 * @Sources2D/correlation_pnr_parallel.m:70-104 -> endoscope/correlation_image_endoscope.m:36-96 -> utilities/correlation_image.m:31-77:
 *   HY = imfilter(Y, psf, 'replicate') (border replicated at the BLOCK edge);  HY -= median(HY, 2);  PNR = max(HY, [], 2) ./ GetSn(HY);
 *   HY(HY < sig * Sn) = 0;  Cn = the mean correlation of every pixel's trace with its 8 neighbours inside the block.
 * psf: psf_n x psf_n, column-major, psf_n odd and <= 25 (an even kernel is zero-padded by the caller: sources2d.seed_psf); NULL / 0 = no filter (gSig <= 0).
 * Q: nframes x M orthonormal columns (column-major, M <= 16) spanning the detrend basis of detrend_data.m:23 (nk > 1, method 'spline'): the filtered trace
 * loses its projection on them first; NULL / 0 = no detrending.  sig: the threshold factor (the reference's is 3).
 * Frames [frame0, frame0 + nframes) with frame0 == 0 and 64 <= nframes <= min(T, 147456) (WELCH_TMAX, the longest trace the Welch estimator takes); anything
 * else, and a derived (bg_ssub) patch, is CNMFE_EUNSUPPORTED.  Up to 20416 frames a pixel's trace and its Welch transform share one workgroup's LDS; beyond, the
 * statistics kernel keeps the trace in a row of the context's scratch (at most 1024 rows of 4 * ceil4(nframes) bytes, 256 from 36869 frames on: <= 151 MB, plus
 * 12 * nfft bytes of transform tables per row from there on), which stays with the context.  The block is filtered whole (the reference's 500^3-sample sub-patch split of :50-59 is a memory workaround and is not reproduced).
 * Scratch: the filtered block, 16 * ceil(nframes / 4) * d_b bytes, allocated for the call and released before it returns (CNMFE_ENOMEM names the bytes);
 * no resident state of the patch is read or written except the centred video.  Two calls return bit-identical images.  A pixel without a neighbour inside the
 * block (a 1 x 1 block) has Cn = 0 / 0 = NaN, as in the reference; a constant trace (Sn = 0) has PNR = NaN likewise.  Outputs: d_b floats each, the patch's
 * caller keeps the patch interior (:108-128). */
int cnmfe_seed_images(cnmfe_ctx *ctx, int patch_id, const float *psf, int32_t psf_n, int64_t frame0, int64_t nframes,
                      const double *Q, int32_t M, float sig, float *Cn_block /* d_b */, float *PNR_block /* d_b */);

/* ---- (g) greedy initialisation: the peel-off of greedyROI_endoscope as a session per patch
 * endoscope/greedyROI_endoscope.m:119-145 (open), :287-311 + endoscope/extract_ac.m:19-58 (extract), :378-402 (apply).  The loop over the seed pixels, the
 * images v_search / ind_search, the shape constraints and the baseline fit are the host's (sources2d.Sources2D.initComponents_parallel); one step's work over
 * a pixel box times all frames is the device's.
 *
 * cnmfe_peel_open: the arguments, refusals and the images Cn_block / PNR_block of cnmfe_seed_images (bit-identical), plus Sn_block = GetSn of the filtered
 * traces (d_b floats, may be NULL).  The session keeps HY (the filtered block, trend and median subtracted: :130), Sn in fp64 (:132) and Yw, a working copy of the
 * centred video (M > 0: of the detrended video), 2 x 16 * ceil(nframes / 4) * d_b bytes; CNMFE_ENOMEM if they do not fit, CNMFE_ESTATE if the patch already
 * has a session.  The resident video and all fit state stay untouched.
 *
 * cnmfe_peel_extract: the seed (r, c), 0-BASED in the block; box = rows max(0, r - gSiz) .. min(nr_b - 1, r + gSiz), columns likewise (:299-300), nr x nc
 * pixels column-major.  corr_box = Pearson's r of every box pixel's HY trace with the seed's (NaN for a constant trace); ci = mean of HY over {corr > 0.9}
 * (nframes doubles); y_bg(t) = the exact median over {corr < 0.3} of Yw + the pixel mean (M > 0: of Yw), NaN for an empty set; ai_box = row 3 of
 * ([1, y_bg, ci]' [1, y_bg, ci]) \ ([1, y_bg, ci]' Y') clipped at 0 (max(0, NaN) = 0), before any constraint.  stats[6] = max(diff(y0)), std(diff(y0)),
 * norm(ci), GetSn(ci), |{corr > 0.9}|, |{corr < 0.3}|.  Nothing of the session changes.
 *
 * cnmfe_peel_apply: Yw(box) -= ai_box ci (:378); HY(box2) -= Hai_box2 ci (:385-387) on box2 = the box of reach 2 gSiz (:310-311); then per box2 pixel
 * PNR_box2 = max(HY) / Sn (NaN or < min_pnr -> 0, :391-393) and Cn_box2 = the 8-neighbour correlation image of HY(box2) thresholded at sig Sn, the box
 * taken as a whole image (:396-401; NaN or < min_corr -> 0).
 *
 * cnmfe_peel_open_residual: the session of the SECOND pass (@Sources2D/initComponents_residual_parallel.m:186-220), on the PATCH (nr x nc, d pixels) and on
 *   Yres = Ysig - A(patch, ind) C(ind, :)                                                   (:199 on the patch rows, after :206 / :209-217)
 * with Ysig the resident residual of cnmfe_residual / cnmfe_residual_ssub (called with the block's current neurons; CNMFE_ESTATE without one, a recorded or
 * pending one is realised first, as for cnmfe_get_sn).  A: d x Ksel CSC over the PATCH rows (empty columns are legal: a neuron that only touches the halo), C as
 * for cnmfe_residual; Ksel = 0 searches Ysig itself.  Per pixel the stored neurons are summed in fp64 in ascending column order and the difference is rounded
 * once to fp32; Ysig is only read.  All T frames are used (64 <= T <= 147456, as cnmfe_seed_images), there is no detrending (M = 0), y_bg takes no pixel mean (the residual carries its
 * own), and extract / apply take the seed 0-BASED in the PATCH and clip their boxes at the patch (tmp_options.d1 / d2, :176-177).  Cn_patch / PNR_patch /
 * Sn_patch: d floats (Sn may be NULL); Yres_out (may be NULL): exactly the fp32 video the session searches, d x T frame-major like cnmfe_residual's output, to
 * host or device memory (out_memspace).  The session keeps 2 x 16 * ceil(T / 4) * d bytes (HY and Yw, which starts as Yres; CNMFE_ENOMEM names them).  The
 * residual request belongs to the session: cnmfe_peel_close -- and an open that fails after the residual was realised -- drops it as a background fit does
 * (a NEW side effect of cnmfe_peel_close, for residual sessions only), so the next update requests its own and sees the patch as it would have without the
 * session; W, b0 and every table of the fit stay untouched.
 *
 * gSiz > 20 is CNMFE_EUNSUPPORTED; extract / apply / close without a session are CNMFE_ESTATE, a seed outside the session's geometry is CNMFE_EINVAL.  Every reduction runs in a fixed order: two identical
 * sessions are bit-identical.  The calls run on the patch's lane. */
int cnmfe_peel_open(cnmfe_ctx *ctx, int patch_id, const float *psf, int32_t psf_n, int64_t frame0, int64_t nframes,
                    const double *Q, int32_t M, float sig, float *Cn_block /* d_b */, float *PNR_block /* d_b */, float *Sn_block /* d_b or NULL */);
int cnmfe_peel_open_residual(cnmfe_ctx *ctx, int patch_id, int32_t Ksel, const int64_t *A_colptr, const int32_t *A_rowidx /* in [0, d) */, const float *A_val,
                             const float *C, int c_order, const float *psf, int32_t psf_n, float sig, float *Cn_patch /* d */, float *PNR_patch /* d */,
                             float *Sn_patch /* d or NULL */, float *Yres_out /* d x T or NULL */, int out_memspace);
/* options.ssub / options.tsub (greedyROI_endoscope.m:46-61, correlation_pnr_parallel.m:81-100): the same two calls on Yds = dsData(Y) of the block
 * (utilities/dsData.m:29-43), which is built on the device from the resident centred video in one pass:
 *   spatial   per frame imresize(., [d1s, d2s], 'box') with d1s = ceil(nr_b / ssub), d2s = ceil(nc_b / ssub): the box kernel stretched by in / out PER
 *             DIMENSION (antialiasing), taps mirrored at the border, each row of weights normalised (a size ssub does not divide has a scale that is not 1 / ssub);
 *   temporal  the mean of every tsub consecutive frames, Ts = floor(nframes / tsub), the rest discarded.
 * Taps then frames are summed in fp64 in a fixed order and rounded once to fp32; two calls are bit-identical.  ssub in 1 .. 8 and tsub >= 1, else
 * CNMFE_EINVAL; floor(nframes / tsub) < 64 and a derived (bg_ssub) patch are CNMFE_EUNSUPPORTED; otherwise the refusals of cnmfe_seed_images (frame0 = 0).
 *
 * cnmfe_seed_images_ds (correlation_pnr_parallel.m:86-96): down-sample first, then the seed pipeline on the SHORT series -- Q is Ts x M.  The caller scales the
 * filter (gSig / ssub, ceil(gSiz / ssub)) and resizes the d1s x d2s images back.  Scratch of the call: the down-sampled and the filtered video, 2 x 16 *
 * ceil(Ts / 4) * d1s d2s bytes.
 *
 * cnmfe_peel_open_ds: the session on the d1s x d2s grid with Ts frames.  Qpre: nframes x Mpre, the FULL-LENGTH detrend basis (initComponents_parallel.m:341-343
 * detrends the full block before greedyROI_endoscope.m:52 down-samples it); the two maps commute in exact arithmetic, so the device projects the spatially
 * resized pixels on Qpre (k_ds_coef) and subtracts the bin means of the trend inside the down-sampling pass: no full-resolution detrended copy exists.  The seed
 * pipeline then runs with M = 0.  Yw starts as the down-sampled video (Yds_out, may be NULL: exactly that fp32 video, d1s d2s x Ts frame-major, to host or device
 * memory); y_bg adds box(pixel mean), with Mpre > 0 nothing.  The session keeps 2 x 16 * ceil(Ts / 4) * d1s d2s bytes (CNMFE_ENOMEM names them).
 * cnmfe_peel_extract / _apply / _close work in the session's geometry: seeds 0-based on the d1s x d2s grid, ci of Ts samples.  ssub = tsub = 1, Mpre = 0 is the
 * identity: Yds_out is the centred video bit for bit and the images are cnmfe_peel_open's.
 *
 * cnmfe_peel_open_residual_ds: options.ssub / options.tsub of the SECOND pass (initComponents_residual_parallel.m:171-177,232 hands greedyROI_endoscope the
 * patch residual, which :46-61 down-samples): the session on dsData(Yres) of the PATCH, d1s = ceil(nr / ssub), d2s = ceil(nc / ssub), Ts = floor(T / tsub).
 * dsData is linear, so the device forms
 *   dsData(Ysig - A C) = dsData(Ysig) - A_ds C_ds
 * off the resident residual: A_ds = every footprint column box-resized on the patch grid (the library does it in float64 with the tap tables of the kernel,
 * exact zeros dropped), C_ds = the mean of every tsub consecutive samples of each trace (on the device in fp64: a bound C never comes down).  Per low-resolution
 * pixel and frame: taps, then the frames of the bin in ascending order, one division by tsub, then the pixel's footprints in ascending column order by fma, ONE
 * rounding to fp32 -- no full-resolution difference video exists and two calls are bit-identical.  Arguments and refusals are those of cnmfe_peel_open_residual
 * (A over the PATCH rows at FULL resolution, the resident residual, no open session, no derived patch) plus the factors': ssub in 1 .. 8 and tsub >= 1, else
 * CNMFE_EINVAL; floor(T / tsub) < 64 is CNMFE_EUNSUPPORTED.  Cn_ds / PNR_ds / Sn_ds: d1s d2s floats; Yds_out (may be NULL): exactly the fp32 video the
 * session searches, d1s d2s x Ts frame-major.  The session keeps 2 x 16 * ceil(Ts / 4) * d1s d2s bytes (CNMFE_ENOMEM names them); extract / apply take seeds
 * 0-based on the d1s x d2s grid and ci of Ts samples; y_bg takes no pixel mean.  The residual request belongs to the session exactly as for
 * cnmfe_peel_open_residual (cnmfe_peel_close and a failed open drop it).  ssub = tsub = 1 IS cnmfe_peel_open_residual: images, Sn and video bit for bit. */
int cnmfe_seed_images_ds(cnmfe_ctx *ctx, int patch_id, int32_t ssub, int32_t tsub, const float *psf, int32_t psf_n, int64_t nframes,
                         const double *Q /* Ts x M */, int32_t M, float sig, float *Cn_ds /* d1s * d2s */, float *PNR_ds /* d1s * d2s */);
int cnmfe_peel_open_ds(cnmfe_ctx *ctx, int patch_id, int32_t ssub, int32_t tsub, const float *psf, int32_t psf_n, int64_t nframes,
                       const double *Qpre /* nframes x Mpre */, int32_t Mpre, float sig, float *Cn_ds /* d1s * d2s */, float *PNR_ds /* d1s * d2s */,
                       float *Sn_ds /* d1s * d2s or NULL */, float *Yds_out /* d1s * d2s x Ts or NULL */, int out_memspace);
int cnmfe_peel_open_residual_ds(cnmfe_ctx *ctx, int patch_id, int32_t ssub, int32_t tsub, int32_t Ksel, const int64_t *A_colptr,
                                const int32_t *A_rowidx /* in [0, d) */, const float *A_val, const float *C, int c_order, const float *psf, int32_t psf_n, float sig,
                                float *Cn_ds /* d1s * d2s */, float *PNR_ds /* d1s * d2s */, float *Sn_ds /* d1s * d2s or NULL */,
                                float *Yds_out /* d1s * d2s x Ts or NULL */, int out_memspace);
int cnmfe_peel_extract(cnmfe_ctx *ctx, int patch_id, int32_t r, int32_t c, int32_t gSiz, double *corr_box /* nr * nc */, double *ai_box /* nr * nc */,
                       double *ci /* nframes */, double *stats /* 6 */);
int cnmfe_peel_apply(cnmfe_ctx *ctx, int patch_id, int32_t r, int32_t c, int32_t gSiz, const double *ai_box /* nr * nc */,
                     const double *Hai_box2 /* nr2 * nc2 */, const double *ci /* nframes */, double sig, double min_pnr, double min_corr,
                     float *PNR_box2 /* nr2 * nc2 */, float *Cn_box2 /* nr2 * nc2 */);
int cnmfe_peel_close(cnmfe_ctx *ctx, int patch_id);

/* sn of the BLOCK pixels of a patch (obj.P.sn(logical(mask)), update_background_parallel.m:131; for a low-resolution fit patch of
 * bg_ssub > 1 the resized values of :137).  Only the outlier branch of the ring fit reads them. */
int cnmfe_set_noise(cnmfe_ctx *ctx, int patch_id, const float *sn_block /* d_b */);

/* ---- bg_ssub > 1: the ring model on a spatially downsampled block
 * W lives on the ceil(nr_b/s) x ceil(nc_b/s) grid with ring radius ceil(r/s)  (@Sources2D/initComponents_parallel.m:214,237-251).
 * cnmfe_patch_derive creates a patch whose FOV is that grid and whose resident video is computed on the device from the
 * source patch: CNMFE_DERIVE_NEAREST = imresize(., 1/s, 'nearest') (what fit_ring_model sees, update_background_parallel.m:224),
 * CNMFE_DERIVE_BICUBIC = imresize(., 1/s) of the centred video (what W multiplies, update_spatial_parallel.m:171-172).
 * Call cnmfe_ring_init(new_patch, ceil(r/s), num_neighbors) on both afterwards. */
enum { CNMFE_DERIVE_NEAREST = 0, CNMFE_DERIVE_BICUBIC = 1 };
int cnmfe_patch_derive(cnmfe_ctx *ctx, int src_patch, int new_patch, int32_t ssub, int mode);

/* update_background_parallel.m:219-230:  b0 = mean(Y - A*C, 2)(patch);  W = fit_ring_model(imresize(Y - A*C, 1/s, 'nearest'), [], [], W_old, ...).
 * A is d_b x K CSC over BLOCK rows of patch_id; W is fitted on fit_patch and copied to res_patch; b0 is set on patch_id.  info as in
 * cnmfe_fit_ring_model (of the low-resolution fit). */
int cnmfe_fit_ring_model_ssub(cnmfe_ctx *ctx, int patch_id, int fit_patch, int res_patch, int32_t ssub, int32_t K,
                              const int64_t *A_colptr, const int32_t *A_rowidx, const float *A_val, const float *C, int c_order,
                              double thresh_outlier, int with_projection, int64_t info[4]);

/* update_spatial_parallel.m:167-178 == update_temporal_parallel.m:153-165:
 *   Ysig = Y(ind_patch,:) - imresize(W * imresize(R - mean(R,2), 1/s), [nr_block nc_block])(ind_patch,:) - b0,  R = Y - A_prev*C_prev.
 * The result stays resident as the Ysig of patch_id (for cnmfe_update_spatial / cnmfe_hals_temporal / cnmfe_get_sn).
 * Round 5: with Ysig_out == NULL the request is only RECORDED (as cnmfe_residual does since round 4; option ssub_virtual): cnmfe_update_spatial and
 * cnmfe_hals_temporal take Ysig*C' and A'*Ysig through the two resampling maps from the video rows under the masks / footprints and the low-resolution video of
 * res_patch (fp64 sums); every other consumer runs the low-resolution sweep and its upsample first.  res_patch must stay alive until the next fit / upload. */
int cnmfe_residual_ssub(cnmfe_ctx *ctx, int patch_id, int res_patch, int32_t ssub, int32_t Ksel, const int64_t *A_colptr,
                        const int32_t *A_rowidx, const float *A_val, const float *C, int c_order,
                        float *Ysig_out /* d x T or NULL */, int out_memspace);

/* ---- R1: the residual / background-subtraction expression
 *   Ysig = Y(ind_patch,:) - W*(Y - A_prev*C_prev) - (b0 - W*mean(Y - A_prev*C_prev, 2))
 * update_spatial_parallel.m:162-166 == update_temporal_parallel.m:149-152.
 * A_prev is d_b x Ksel CSC (block rows), C_prev Ksel x T.  The result (d x T fp32,
 * frame-major) stays resident for the HALS/NNLS calls below; Ysig_out may be NULL, and then
 * the call returns with the sweep still running on the context's stream (all inputs have been
 * consumed; later calls on this context are stream-ordered behind it and report its errors).
 * Ysig stays resident PER PATCH.  While the video, W and b0 of the patch are unchanged, a further call only changes the footprint
 * term (W*A_prev)*(C_prev - mean): the difference is folded into the resident Ysig in one streaming pass (option "r1_delta",
 * default 1), or merely recorded (option "r1_lazy", default 1) -- cnmfe_hals_temporal[_deconv] then adds A'*(W*A_prev)*(C_prev - mean)
 * to A'*Ysig without another pass over the video, every other consumer folds it in first.  The values any caller sees are those of
 * the full expression above (up to fp32 rounding of the re-association).
 * Option "r1_defer" (default 1; ring radius 15, no Ysig_out): the FIRST residual after a fit also runs its sweep without the footprint term and leaves
 * the term pending -- cnmfe_update_spatial adds (W*A_prev)*((C_prev - mean)*(C - mean)') to its projection Ysig*C' on the search mask, so patches with
 * halo neurons are swept by the same (fastest) kernel as a patch without. */
int cnmfe_residual(cnmfe_ctx *ctx, int patch_id, int32_t Ksel, const int64_t *A_colptr,
                   const int32_t *A_rowidx, const float *A_val, const float *C, int c_order,
                   float *Ysig_out, int out_memspace);

/* ---- S5: sn = GetSn(Ysig) of every patch pixel (update_sn = true)
 * @Sources2D/update_spatial_parallel.m:191-194 -> OASIS_matlab/functions/GetSn.m:33-47
 * (Welch PSD with pwelch's defaults, sn = sqrt(exp(mean(log(psd/2)))) over 0.25 <= f <= 0.5).
 * Ysig = the resident residual of this patch (cnmfe_residual must have been called).  sn_out: d floats. */
int cnmfe_get_sn(cnmfe_ctx *ctx, int patch_id, float *sn_out);

/* ---- S1-S4: A = HALS_spatial(Y,A,C,active_pixel,maxIter)            utilities/HALS_spatial.m:1-45
 *             A = HALS_spatial_thresh(Y,A,C,active_pixel,maxIter,sn)  utilities/HALS_spatial_thresh.m:1-53
 *             A = nnls_spatial(Y,A,C,active_pixel,maxN)               endoscope/nnls_spatial.m:1-109
 * Y = the resident Ysig of this patch (cnmfe_residual must have been called).
 * A is d x K CSC over PATCH rows, IND (active_pixel) d x K CSC pattern, sn d floats
 * (HALS_THRESH only).  param = maxIter (HALS*) or maxN (NNLS).  The result has exactly
 * the IND pattern: A_out[nnz(IND)] in IND's CSC order (entries may be 0).
 * A_out == NULL defers the download: the call returns with the sweeps queued and cnmfe_update_spatial_fetch(ctx, A_out, nnz(IND)) collects the
 * values later -- the host mirror sets up the temporal update's residual in between.  The deferred result is valid until the next spatial, temporal
 * (cnmfe_hals_temporal[_deconv]), fast-temporal or post-processing call on the same lane (option lanes; one lane: of this context): those calls reuse the scratch
 * it lies in, and a fetch after one of them returns CNMFE_ESTATE.  cnmfe_deconv_temporal reuses the mask's pattern only: cnmfe_update_spatial_fetch[_async] still
 * serve after it, the connected fetches below do not.  cnmfe_hals_temporal_job works in buffers of its own and leaves the result alone. */
int cnmfe_update_spatial(cnmfe_ctx *ctx, int patch_id, int algorithm, int32_t K,
                         const int64_t *A_colptr, const int32_t *A_rowidx, const float *A_val,
                         const float *C, int c_order,
                         const int64_t *IND_colptr, const int32_t *IND_rowidx,
                         const float *sn, int32_t param, float *A_out);
int cnmfe_update_spatial_fetch(cnmfe_ctx *ctx, float *A_out, int64_t nnz);
/* the same fetch without the wait: the copy into PINNED host memory (cnmfe_host_alloc; a kernel writes it through the mapping, in 16-byte units: room for nnz floats
 * rounded up to 16 bytes) is queued behind the sweeps and *ticket names the point of the
 * stream where it is complete; cnmfe_ticket_wait(ctx, ticket) waits for exactly that point (not for what was queued after it) and releases the ticket.
 * With several patches per context the host mirror queues patch m + 1 before it collects patch m, so the device never waits for the host's assembly
 * of A (update_spatial_parallel.m:324-334).  A kernel-raised error is reported by the next waiting call of the context, not by the ticket. */
int cnmfe_update_spatial_fetch_async(cnmfe_ctx *ctx, float *A_out_pinned, int64_t nnz, int64_t *ticket);
int cnmfe_ticket_wait(cnmfe_ctx *ctx, int64_t ticket);
/* the same fetch with post_process_spatial's connectivity constraint (cnmfe_post_process_spatial below) applied to the result where it lies on the
 * device: for a patch that IS the d1 x d2 field of view (patch rows = FOV pixels), IND = the mask the deferred update ran on.  A_out = the raw update
 * (obj.A before post-processing), keep_out[e] = 1 where entry e survives. */
int cnmfe_update_spatial_fetch_connected(cnmfe_ctx *ctx, int32_t d1, int32_t d2, int32_t K, const int64_t *IND_colptr, const int32_t *IND_rowidx,
                                         float *A_out, uint8_t *keep_out);

/* the connected fetch without the wait: the connectivity kernel and the two copies into PINNED memory (cnmfe_host_alloc) are queued, *ticket names the point of
 * the stream where they are complete (cnmfe_ticket_wait).  The host mirror queues the temporal update's residual request behind it -- whatever that request starts
 * on the device (the deferred half of the ring solve, the W*A_prev tables) then runs while the host turns the result into the next call's A. */
int cnmfe_update_spatial_fetch_connected_async(cnmfe_ctx *ctx, int32_t d1, int32_t d2, int32_t K, const int64_t *IND_colptr, const int32_t *IND_rowidx,
                                               float *A_out_pinned, uint8_t *keep_out_pinned, int64_t *ticket);

/* ---- fast_temporal (use_c_hat = false)                @Sources2D/update_temporal_parallel.m:174-175,314-337
 *   tmp_A = A .* (A ./ max(A,[],1) >= 0.5);  aa = sum(tmp_A.^2,1);  C_raw = (tmp_A' * Ysig) ./ aa'
 * (rows with aa == 0 are 0 and report aa = 0).  A is d x K CSC over PATCH rows; Ysig = the resident
 * residual of this patch.  C_raw_out K x T (NULL: keep the result on the device for cnmfe_stitch_add), aa_out K floats (may be NULL). */
int cnmfe_fast_temporal(cnmfe_ctx *ctx, int patch_id, int32_t K, const int64_t *A_colptr,
                        const int32_t *A_rowidx, const float *A_val, int c_order,
                        float *C_raw_out, float *aa_out);

/* ---- T1-T3: [C, C_raw, ~, ~] = HALS_temporal(Y, A, C, maxIter, [])   utilities/HALS_temporal.m:1-119
 * (no-deconvolution branch :64-68).  Y = resident Ysig.  A d x K CSC over PATCH rows.
 * Outputs in c_order (each may be NULL: C_raw and aa also stay on the device for cnmfe_stitch_add); aa_out[k] = sum(A(:,k).^2)
 * (update_temporal_parallel.m:181). */
int cnmfe_hals_temporal(cnmfe_ctx *ctx, int patch_id, int32_t K, const int64_t *A_colptr,
                        const int32_t *A_rowidx, const float *A_val, const float *C_in, int c_order,
                        int32_t maxIter, float *C_out, float *C_raw_out, float *aa_out);

/* ---- T4/T6: deconvolution (options.deconv_flag = true) ---------------------------------------
 * deconv_options of demos/demo_large_data_1p.m:38-43; only type 'ar1' + method 'foopsi' is built. */
typedef struct cnmfe_deconv_opts {
    int32_t type;            /* 1 = 'ar1' */
    int32_t method;          /* 1 = 'foopsi' */
    double  smin;            /* negative: |smin| * noise level (deconvolveCa.m:116-118) */
    double  lambda;          /* must be 0 */
    double  max_tau;         /* gmax = exp(-1/max_tau) (deconvolveCa.m:119) */
    int32_t optimize_b;
    int32_t optimize_pars;
    int32_t maxIter;         /* deconvTemporal only (default 10); HALS_temporal forces 20 (HALS_temporal.m:92) */
} cnmfe_deconv_opts;

/* [C, C_raw, results_deconv] = HALS_temporal(Y, A, C, maxIter, deconv_options)   utilities/HALS_temporal.m:70-104
 * (the deconvolution branch: per row GetSn + deconvolveCa inside the Gauss-Seidel sweep).
 * kernel_pars[K] in/out (0 = not yet estimated), S_out / sn_out receive results_deconv.S / .sn.
 * With C_out, C_raw_out, S_out and sn_out all NULL nothing is copied back -- kernel_pars is then input only -- and the call returns with the sweeps in
 * flight (C_raw and aa stay on the device for cnmfe_stitch_add). */
int cnmfe_hals_temporal_deconv(cnmfe_ctx *ctx, int patch_id, int32_t K, const int64_t *A_colptr,
                               const int32_t *A_rowidx, const float *A_val, const float *C_in, int c_order,
                               int32_t maxIter, const cnmfe_deconv_opts *opts, float *kernel_pars,
                               float *C_out, float *C_raw_out, float *S_out, float *sn_out, float *aa_out);
/* obj.deconvTemporal()  (@Sources2D/deconvTemporal.m:29-105): every row of C_raw (K x T, in/out: the fitted
 * baseline is subtracted) is deconvolved with a fresh time-constant estimate. */
int cnmfe_deconv_temporal(cnmfe_ctx *ctx, int32_t K, int64_t T, float *C_raw, int c_order,
                          const cnmfe_deconv_opts *opts, float *C_out, float *S_out,
                          float *kernel_pars_out, float *sn_out);
/* The same on the BOUND trace matrix (cnmfe_traces_bind, cnmfe_stitch_finish*): the stitched C_raw is deconvolved where it lies, the denoised C becomes
 * the bound matrix (what the next background / spatial / temporal update reads with (NULL, CNMFE_BOUND)), C_raw - b and S stay in the context -- no
 * K x T array crosses PCIe on the critical path.  The host outputs (row-major K x T / K floats, PINNED memory from cnmfe_host_alloc, any may be NULL) are
 * written by a second stream behind the kernels: cnmfe_stitch_wait waits for them.  CNMFE_ESTATE without a bound matrix. */
int cnmfe_deconv_temporal_bound(cnmfe_ctx *ctx, const cnmfe_deconv_opts *opts, float *C_out, float *C_raw_out, float *S_out,
                                float *kernel_pars_out, float *sn_out);

/* ---- (h) merging: the calls of demos/demo_large_data_1p.m:146-147,168,175-178,189,205-207,212 between the updates
 * @Sources2D/merge_high_corr.m:50-85,172-196,236   merge_neurons_dist_corr.m:58-86,180-201,243   merge_close_neighbors.m:49-83,174-195,237
 * @Sources2D/Sources2D.m:744-759 (remove_false_positives -> tag_neurons_parallel :1683-1715)
 * The K x K criteria, graph_connected_comp and the n x n form of a group's alternation are the host's (float64: sources2d.Sources2D.merge_*, hostops.py); everything that
 * is K x T runs here, on the matrices the context already holds: the bound matrix C and, beside it, the RESIDENT C_raw, S, kernel_pars and sn that
 * cnmfe_deconv_temporal_bound leaves (C_raw - b and S "stay in the context").  They belong together until the bound matrix' content changes by any other call.
 * A trace SOURCE (X, src) is: a host pointer with src = CNMFE_COLMAJOR / CNMFE_ROWMAJOR (one upload: counted by the read-only counter merge_trace_uploads of
 * cnmfe_get_option), or X ignored and src = CNMFE_BOUND (C), CNMFE_RES_CRAW, CNMFE_RES_S (the residents), CNMFE_RES_DIFF (the last result of
 * cnmfe_trace_diff_spikes).  K and T must be the source's.  Every reduction runs in a fixed order: two calls on equal inputs are bit-identical, on any GPU. */
enum { CNMFE_RES_CRAW = 4, CNMFE_RES_S = 5, CNMFE_RES_DIFF = 6 };
/* the residents from the host (a caller whose matrices are NOT the context's: deconv_flag = false, a sharded run): C is bound as by cnmfe_traces_bind, C_raw (NULL: C),
 * S (NULL: none -- the context then has no S, cnmfe_trace_tags reports -1 spikes) and kernel_pars (K floats or NULL = 0) become the residents.  Two or three uploads. */
int cnmfe_traces_load(cnmfe_ctx *ctx, int32_t K, int64_t T, const float *C, const float *C_raw, const float *S, const float *kernel_pars, int c_order);
/* out (K x K doubles, symmetric) = corr(X') -- Pearson's r of the rows, merge_high_corr.m:67-68, merge_neurons_dist_corr.m:70 (the caller subtracts eye(K)) -- or, raw != 0,
 * the uncentred Gram X X' (its sub-blocks are the G of a group's alternation :176-181).  Mean and centred sum of squares per row in fp64, the products on the fp64 matrix
 * pipe with the fp64 mean subtracted from every operand.  A row without variance gives NaN in its row and column (MATLAB's 0 / 0).  K = 0 is legal. */
int cnmfe_trace_corr(cnmfe_ctx *ctx, int32_t K, int64_t T, const float *X, int src, int raw, double *out);
/* merge_high_corr.m:57-66, the branch without S:  S_ = diff(X, 1, 2);  S_(:, end + 1) = 0;  S_(S_ < 2 * GetSn(S_)) = 0  with GetSn per row (fp32 differences, the Welch
 * estimator of the traces).  The result stays in the context as the source CNMFE_RES_DIFF; sn_out (K floats) and S_out (K x T ROW-MAJOR) may be NULL.  64 <= T <= 147456
 * (WELCH_TMAX; beyond 20416 frames the difference trace lives in its output row, not in LDS: the long flavour, bit-equal where both run). */
int cnmfe_trace_diff_spikes(cnmfe_ctx *ctx, int32_t K, int64_t T, const float *X, int src, float *sn_out, float *S_out);
/* tag_neurons_parallel's per-trace quantities (Sources2D.m:1700-1709) of the context's C, C_raw, S, one workgroup per trace, one pass:
 * out[4 k + 0] = max(C(k, :)), [1] = std(C_raw(k, :) - C(k, :), 0) in fp64, [2] = GetSn(C_raw(k, :)), [3] = |{t >= 2 : S(k, t) > 0}| (-1 without an S).
 * K must be the bound matrix'; the bit arithmetic (and nnz(A(:, k)) < min_pixel) is the host's.  64 <= T <= 147456 (WELCH_TMAX; beyond 20416 frames
 * C_raw's row is read in place). */
int cnmfe_trace_tags(cnmfe_ctx *ctx, int32_t K, double *out /* 4 K */);
/* orderROIs' per-trace statistics (Sources2D.m:573-653) and the max(CC, [], 2) of show_demixed_video.m:37, of the context's C and C_raw, one workgroup per trace, fp64,
 * two passes (the means first), a fixed reduction order:
 * out[7 k + 0] = mean(C(k, :)), [1] = var(C(k, :), 0), [2] = var(C_raw(k, :) - C(k, :), 0), [3] = max(C(k, :)), [4] = ||C_raw(k, :)||_2, [5] = ||C_raw(k, :)||_1,
 * [6] = max(C_raw(k, :)).  K must be the bound matrix' (CNMFE_ESTATE otherwise, or without residents); K = 0 is legal.  T is a loop bound: any T >= 1. */
int cnmfe_trace_order_stats(cnmfe_ctx *ctx, int32_t K, double *out /* 7 K */);
/* The K-changing step of the three merges and of obj.delete, in place on the context's matrices (K rows before, nkeep after):
 *   group g = rows grp_idx[grp_ptr[g] .. grp_ptr[g + 1]) with weights w[...] (same positions): ci = w' C_raw(IDs, :) summed in fp64 in that order and rounded to fp32
 *   once is the new C_raw row of IDs(1) = its first member (:184); deconvolveCa(ci, deconv_options_0) by the AR(1) FOOPSI kernel of cnmfe_deconv_temporal with a fresh
 *   time constant gives the row's C, S, kernel_pars and sn (:187-188; C_raw keeps ci itself -- the reference subtracts no baseline here);
 *   then rows keep[0 .. nkeep) (distinct, any order; every group's first member among them, its other members normally not) are gathered into new matrices:
 *   obj.delete(ind_del) (:236).  The compacted C becomes the bound matrix (row-major, as cnmfe_traces_bind would make it), C_raw / S / kernel_pars / sn the residents.
 * ngroups = 0 (opts may be NULL) is the device-side delete.  Host outputs (nkeep x T row-major, nkeep floats) may each be NULL; the call returns when they are written.
 * A merged trace without a stable AR(1) model or without any spike gets C = C_raw - b as in deconvTemporal.m:53-55 (the reference's deconvolveCa returns zeros).
 * CNMFE_ESTATE without residents, CNMFE_EINVAL on an index out of range, a repeated kept row, an empty group or a group whose first member is not kept. */
int cnmfe_merge_apply(cnmfe_ctx *ctx, int32_t ngroups, const int32_t *grp_ptr, const int32_t *grp_idx, const double *w, int32_t nkeep, const int32_t *keep,
                      const cnmfe_deconv_opts *opts, float *C_out, float *C_raw_out, float *S_out, float *kernel_pars_out, float *sn_out);
/* Batch mode (demos/demo_batch_1p.m:120-142; cnmf_e_amd/batch.py): several recordings of one field of view, one context each, share the footprints.  Two calls keep a
 * batch method from moving a K x T matrix that already lies in HBM.
 * out[k] (K doubles) = sum_t X(k, t)^2, the weight of a batch in the footprint average (update_spatial_batch.m:29), of a trace SOURCE as above (CNMFE_RES_DIFF included).
 * One pass, fp64 sums in a fixed order without atomics: the bits do not depend on the option lanes or on the call.  T >= 1 (no Welch estimate is taken); K = 0 is legal. */
int cnmfe_trace_energy(cnmfe_ctx *ctx, int32_t K, int64_t T, const float *X, int src, double *out);
/* obj.C = [obj.C; zeros(K_new - K, T)] (initComponents_batch.m:103-106, update_temporal_batch.m:24-27) on the BOUND matrix, on the device: K_new - K zero rows are
 * appended; while the residents C_raw, S, kernel_pars, sn belong to it they grow the same way (zero rows / entries) and go on belonging to it.  The old rows keep their
 * bits, the layout the matrix was bound in stays, nothing is uploaded (the counter trace_matrix_uploads does not move).  K_new == K does nothing.
 * CNMFE_ESTATE without a bound matrix, CNMFE_EINVAL for K_new < K. */
int cnmfe_traces_grow(cnmfe_ctx *ctx, int32_t K_new);

/* ---- T5: the overlap-region stitch of the temporal update, on the device
 * @Sources2D/update_temporal_parallel.m:264-280:
 *     C_new(ind_m, :) += aa_m .* C_raw_m;  aa(ind_m) += aa_m   over the patches m;   C_raw = C_new ./ aa  (aa == 0 -> 1);
 *     without deconvolution  C_raw = C_raw - min(C_raw, [], 2),  C = C_raw   (:285-286)
 * cnmfe_hals_temporal[_deconv] / cnmfe_fast_temporal leave their C_raw rows and aa on the device (their host outputs may be NULL); the
 * stitch accumulates them there, so the K_m x T pieces never cross PCIe:
 *   cnmfe_stitch_begin(ctx, K, T)             zero the accumulator: K rows of (T + weight) floats
 *   cnmfe_stitch_add(ctx, K_m, ind_m)         after each patch's temporal call: rows ind_m (0-based, distinct) += aa_m .* C_raw_m
 *   cnmfe_stitch_temporal(ctxs, n, ...)       the exchange + :279-286.  n contexts of ONE process (one per GPU, each holding the sum over its own
 *                                             patches): RCCL all-reduce (sum) of the accumulators over xGMI, in place; every context then
 *                                             divides, subtracts the row minima if asked, and BINDS the result as its trace matrix
 *                                             (cnmfe_traces_bind semantics, row-major): the next background / spatial update reads it with
 *                                             (NULL, CNMFE_BOUND).  C_raw_out (K x T, c_order; may be NULL) receives a host copy from ctxs[0].
 *   one process PER GPU (torch.distributed, MPI): cnmfe_stitch_buffer hands out the accumulator's device address for the caller's own
 *   all-reduce (count = K * ld floats), cnmfe_stitch_finish does :279-286 + bind on this context. */
int cnmfe_stitch_begin(cnmfe_ctx *ctx, int32_t K, int64_t T);
int cnmfe_stitch_add(cnmfe_ctx *ctx, int32_t K_m, const int32_t *ind_m);
/* Several patches per context: cnmfe_hals_temporal_job does everything cnmfe_hals_temporal[_deconv] does up to the Gauss-Seidel sweeps (opts == NULL: the
 * no-deconvolution branch; kernel_pars: K time constants in, with opts) and keeps the patch's buffers as job *job_out (numbered from cnmfe_stitch_begin);
 * cnmfe_temporal_jobs_sweep runs level l of EVERY job in one launch -- the patches are independent (update_temporal_parallel.m:112-186 is a parfor), and one
 * patch's level is a handful of workgroups as long as one trace's work; cnmfe_stitch_add_job(job, ...) then adds that job's aa .* C_raw to the accumulator.
 * Same values as the per-patch calls (the same kernels on the same operands). */
int cnmfe_hals_temporal_job(cnmfe_ctx *ctx, int patch_id, int32_t K, const int64_t *A_colptr, const int32_t *A_rowidx, const float *A_val,
                            const float *C_in, int c_order, int32_t maxIter, const cnmfe_deconv_opts *opts, const float *kernel_pars, int32_t *job_out);
int cnmfe_temporal_jobs_sweep(cnmfe_ctx *ctx);
int cnmfe_stitch_add_job(cnmfe_ctx *ctx, int32_t job, int32_t K_m, const int32_t *ind_m);

/* ---- (f) known footprints: the traces of given footprints and a given ring background on ANOTHER recording
 * @Sources2D/initTemporal.m:89-168 (ring branch) -> utilities/HALS_temporal.m:34-41 (the rough start without a C), :48-68, :70-104:
 *     AA = sum(A(patch, :).^2, 1)                                                                  (:160, the stitch weight)
 *     Yt = Y(patch, :) - W Y(block, :);   At = A(patch, :) - W A                                   (:165-166: the raw video; no b0, no mean, no previous factors)
 *     [~, C] = HALS_temporal(Yt, At, [], iters_plain);   [C, C_raw, deconv] = HALS_temporal(Yt, At, C, iters_last, deconv_options)       (:167-168; 10 and 2)
 * Y = the resident block, W = the resident W{m} (cnmfe_ring_set_values / a fit; b0 is not read).  A is d_b x K CSC over BLOCK rows (the neurons with any weight in
 * the block, :106-111; columns that are empty or zero on the patch are legal).  opts == NULL: the last sweeps are plain too (S_out, kernel_pars_out, sn_out must
 * be NULL); else they are the in-sweep AR(1) FOOPSI of cnmfe_hals_temporal_deconv with kernel parameters estimated fresh.  At and V = At' At are formed in fp64
 * from the fp32 A and W; U = At' Yt and the rough start come out of ONE block-tiled pass over the centred video (a constant per row of U or of the starting C
 * changes no output of the plain sweeps: every row update ends in "minus its minimum"; the deconvolution sweeps take GetSn before their baseline goes,
 * HALS_temporal.m:79, and get the raw video's constant At' (E - W) Ymean / aa per row in fp64, for GetSn alone) -- several passes only where a 16 x 16 block meets more than 32
 * neurons' (E - W)' At; all sweeps run on the dependency graph of the non-zeros of V, nothing K x T crosses PCIe in between.  Outputs K x T in c_order
 * (CNMFE_COLMAJOR / CNMFE_ROWMAJOR), K floats; each may be NULL: C_raw and AA also stay on the device, and cnmfe_stitch_add then adds AA .* C_raw (:285 --
 * NOT the regression's own aa).  A row with At(:, k) = 0 keeps its rough start (0) and C_raw = 0.  Every reduction has a fixed order: two calls are bit-identical.
 * CNMFE_ESTATE without a ring, CNMFE_EUNSUPPORTED for a derived (bg_ssub) patch or a ring radius above 24; a refused call changes nothing.  No residual of the
 * patch is read, written or invalidated.
 * cnmfe_init_temporal_job: the same for several patches per context, alongside cnmfe_hals_temporal_job (after cnmfe_stitch_begin): the iters_plain sweeps run at
 * once on the patch's lane, the iters_last (> 0) sweeps are job *job_out of cnmfe_temporal_jobs_sweep; cnmfe_stitch_add_job adds AA .* C_raw.
 * Read-only counters (cnmfe_get_option): init_temporal_levels, the level-kernel launches the last call queued itself (the depth of its schedule);
 * trace_matrix_uploads, the K x T matrices any entry point of the context took through a pointer (a bound matrix or rows of it do not count). */
int cnmfe_init_temporal(cnmfe_ctx *ctx, int patch_id, int32_t K, const int64_t *A_colptr, const int32_t *A_rowidx /* BLOCK rows */, const float *A_val,
                        int32_t iters_plain /* 10 */, int32_t iters_last /* 2 */, const cnmfe_deconv_opts *opts /* NULL: plain */,
                        float *C_out, float *C_raw_out, float *S_out, float *kernel_pars_out, float *sn_out, float *AA_out, int c_order);
int cnmfe_init_temporal_job(cnmfe_ctx *ctx, int patch_id, int32_t K, const int64_t *A_colptr, const int32_t *A_rowidx, const float *A_val, int32_t iters_plain,
                            int32_t iters_last, const cnmfe_deconv_opts *opts, float *AA_out, int32_t *job_out);
int cnmfe_stitch_buffer(cnmfe_ctx *ctx, float **dev_acc, int64_t *ld);
/* cnmfe_stitch_buffer without the drain of the stream: also hands out the hipStream_t the additions are queued on.  A collective enqueued ON that stream (torch:
 * `with torch.cuda.stream(torch.cuda.ExternalStream(ptr)): all_reduce(...)` -- RCCL orders itself behind and in front of the current stream with events) needs
 * no host wait on either side; cnmfe_stitch_finish* follows in stream order. */
int cnmfe_stitch_buffer_stream(cnmfe_ctx *ctx, float **dev_acc, int64_t *ld, void **hip_stream);
int cnmfe_stitch_dims(cnmfe_ctx *ctx, int32_t *K, int64_t *T);   /* the K x T recorded by cnmfe_stitch_begin (CNMFE_ESTATE if no stitch is open): a gateway sizes C_raw_out from these, not from its caller */
int cnmfe_stitch_finish(cnmfe_ctx *ctx, int subtract_min, float *C_raw_out, int c_order);
int cnmfe_stitch_temporal(cnmfe_ctx *const *ctxs, int n, int subtract_min, float *C_raw_out, int c_order);
/* cnmfe_stitch_finish without the wait: the host copy (row-major K x T) is written by a second stream into PINNED memory (cnmfe_host_alloc) and is
 * complete after cnmfe_synchronize(ctx); the call itself returns at once, so the caller can set up the next background fit -- which takes the
 * traces from the device binding this call leaves -- while the temporal kernels and the download are still running. */
int cnmfe_stitch_finish_async(cnmfe_ctx *ctx, int subtract_min, float *C_raw_pinned);
int cnmfe_stitch_wait(cnmfe_ctx *ctx);         /* waits for the downloads of cnmfe_stitch_finish_async only (not for the compute stream) */
/* every asynchronous download batch (cnmfe_stitch_finish_async, cnmfe_deconv_temporal_bound) has a generation number: cnmfe_copy_generation after the call
 * that queued it, cnmfe_copy_wait(ctx, gen) waits for THAT batch only -- a host that releases last iteration's buffers must not wait for this iteration's. */
int cnmfe_copy_generation(cnmfe_ctx *ctx, int64_t *gen);
int cnmfe_copy_wait(cnmfe_ctx *ctx, int64_t gen);
void *cnmfe_host_alloc(size_t bytes);          /* page-locked host memory (NULL + cnmfe_last_error on failure) */
void cnmfe_host_free(void *p);

/* ---- host helper: the reference's sparse row selections `A(mask, ind)` with `ind = find(sum(A(mask, :), 1) > 0)` (@Sources2D/update_spatial_parallel.m:87-91,96-97,
 * update_temporal_parallel.m:136-141, update_background_parallel.m:129-131), which MATLAB's sparse indexing does natively and a host in another language does not.
 * CSC in (colptr / rowidx / val of the whole-FOV matrix), `lut[pixel]` = row inside the selection or -1, `cand` = ascending candidate columns.
 * keep_all = 0: a candidate is kept when its selected values sum to > 0 (double accumulation in storage order); 1: every candidate is kept.
 * Out: out_ind[0..*nkept) the kept columns, out_colptr[0..*nkept], their entries (row = lut value, in storage order) in out_rowidx / out_val (capacity `cap`
 * entries: the candidates' total nnz always suffices).  No device involved; CNMFE_EINVAL on a null argument, unsorted candidates or too small a capacity. */
int cnmfe_csc_select_rows(const int64_t *colptr, const int32_t *rowidx, const float *val, const int32_t *lut, int64_t ncand, const int64_t *cand,
                          int keep_all, int64_t cap, int64_t *out_ind, int64_t *out_colptr, int32_t *out_rowidx, float *out_val, int64_t *nkept);
/* host helper: the CSC matrix (ncol columns) without its stored zeros -- and, with keep != NULL, without the entries whose flag is 0 (the connectivity
 * flags of cnmfe_update_spatial_fetch_connected).  A spatial update returns values on the search mask's pattern, most of them zero; MATLAB's sparse
 * matrices drop them on assignment (update_spatial_parallel.m:324-334).  Outputs sized for nnz(in) always suffice; *nnz_out = entries written. */
/* sources2d.py rows_of twice in one pass (update_temporal_parallel.m:83-91: ind = find(sum(A(block,:),1) > 0), A(block, ind), A(patch, ind)): the candidates whose
 * BLOCK entries sum to > 0 as out_ind, their block entries (local rows lut_block) and their patch entries (lut_patch) as two CSC matrices over the same columns */
int cnmfe_csc_select_block_patch(const int64_t *colptr, const int32_t *rowidx, const float *val, const int32_t *lut_block, const int32_t *lut_patch, int64_t ncand,
                                 const int64_t *cand, int64_t cap, int64_t *out_ind, int64_t *blk_colptr, int32_t *blk_rowidx, float *blk_val,
                                 int64_t *pat_colptr, int32_t *pat_rowidx, float *pat_val, int64_t *nkept);
/* the non-empty columns of a sorted CSC footprint matrix over a d1-row image and the bounding boxes of their entries (0-based image rows / columns): the prefilter
 * of the mask selections of update_*_parallel.m (a neuron whose box misses a patch's block cannot be selected there) */
int cnmfe_csc_bbox(int32_t K, int32_t d1, const int64_t *colptr, const int32_t *rowidx, int64_t *nz, int32_t *rmin, int32_t *rmax, int32_t *cmin, int32_t *cmax, int64_t *nnz_cols);
int cnmfe_csc_drop_zeros(int32_t ncol, const int64_t *colptr, const int32_t *rowidx, const float *val, const uint8_t *keep,
                         int64_t *out_colptr, int32_t *out_rowidx, float *out_val, int64_t *nnz_out);

/* host helper: sum, centre of mass (utilities/com.m:20-28, clamped as :26-28) and second central moments (determine_search_location.m:73) of every footprint =
 * column of the d x K CSC matrix A (pixels column-major in a d1 x d2 image); empty[k] = 1 where the values sum to 0 (:52).  K doubles per output.  The caller
 * takes the 2 x 2 eigendecompositions (:74) and hands the result to cnmfe_search_ellipse.  No device involved. */
int cnmfe_footprint_moments(int32_t K, int32_t d1, int32_t d2, const int64_t *colptr, const int32_t *rowidx, const float *val, double *s_out, uint8_t *empty,
                            double *cmx, double *cmy, double *vxx, double *vxy, double *vyy);
/* host helper: the 'ellipse' search masks IND = determine_search_location(A, 'ellipse', params) (utilities/determine_search_location.m:76-100, call site
 * update_spatial_parallel.m:66) from the per-neuron quantities of :52-82 the caller has computed -- centre of mass (utilities/com.m:20-28), eigenvectors
 * vk = (V11, V21, V12, V22) and eigenvalues clamped to [min_size^2, max_size^2] of the footprint's second moments: pixel (r, c) is in mask k iff
 * sqrt(((r - cmx) V11 + (c - cmy) V21)^2 / d11 + ((r - cmx) V12 + (c - cmy) V22)^2 / d22) <= dist (:84), evaluated in exactly that order in double precision,
 * within R pixels of (floor(cmx), floor(cmy)) and inside the d1 x d2 image; empty[k] != 0: no mask (:102-104).  Outputs: out_colptr[K + 1] (always),
 * out_rowidx (0-based global pixels, ascending per neuron; written only when cap >= the total), *nnz_out = the total: call once with out_rowidx = NULL to size
 * the buffer.  No device involved. */
int cnmfe_search_ellipse(int32_t K, int32_t d1, int32_t d2, const double *cmx, const double *cmy, const double *vk, const double *d11, const double *d22,
                         const uint8_t *empty, double dist, int32_t R, int64_t cap, int64_t *out_colptr, int32_t *out_rowidx, int64_t *nnz_out);

/* host helper: the CSC matrix (nrow x ncol, rows ascending per column) of n (row, column, value) triplets in any order -- the gathered rows of A after the spatial
 * update (update_spatial_parallel.m:324-334: every patch writes its own disjoint rows of A_), assembled in one counting pass + a short sort per column instead of a
 * sort of the whole list.  Outputs: out_colptr[ncol + 1], out_rowidx[n], out_val[n].  CNMFE_EINVAL on an index out of range or a (row, column) given twice. */
int cnmfe_csc_from_triplets(int64_t n, const int32_t *rows, const int32_t *cols, const float *vals, int32_t ncol, int64_t nrow,
                            int64_t *out_colptr, int32_t *out_rowidx, float *out_val);

/* ---- objective: [RSS_total, RSS] = compute_RSS(obj)  (@Sources2D/Sources2D.m:1358-1510), ring model, bg_ssub = 1, one patch, all frames:
 *   RSS = sum((Y(patch,:) - A(patch,:)*C - (W*(Y_block - b0_block - A_prev*C_prev) + b0_new(patch))).^2)
 * The resident residual of this patch must be the one of (A_prev, C_prev) = the block's neurons (cnmfe_residual; :1427-1429, :1475);
 * with it RSS is one read of Ysig.  A: d x K CSC on the PATCH rows, C: K x T; b0_block: reconstruct_b0() on the block
 * (d_b floats, column-major), b0_new: obj.b0_new on the patch (d floats). */
int cnmfe_compute_rss(cnmfe_ctx *ctx, int patch_id, int32_t K, const int64_t *A_colptr, const int32_t *A_rowidx,
                      const float *A_val, const float *C, int c_order, const float *b0_block, const float *b0_new,
                      double *rss_out);

/* Ybg = reconstruct_background(obj, frame_range)  (@Sources2D/Sources2D.m:1247-1355), ring model, bg_ssub = 1, one patch:
 *   Ybg(patch, t) = W*(Y_block - b0_block - A_prev*C_prev)(:, t) + b0_new(patch),  t in [frame0, frame0 + nframes)
 * from the resident residual of (A_prev, C_prev) as for cnmfe_compute_rss.  Ybg_out: d x nframes, frame-major, host or device. */
int cnmfe_reconstruct_background(cnmfe_ctx *ctx, int patch_id, const float *b0_block, const float *b0_new,
                                  int64_t frame0, int64_t nframes, float *Ybg_out, int out_memspace);

/* The same two with bg_ssub > 1 (Sources2D.m:1325-1334 and :1479-1486), where both resizes are 'nearest':
 *   Bf = imresize( W * imresize(Y_block - b0_block - A_prev*C_prev, 1/s, 'nearest'), [nr_block nc_block], 'nearest' )(patch)
 * cnmfe_background_ssub forms W * imresize(...) on the fit patch (the low-resolution patch that holds W; A_prev: d_b x K CSC on the BLOCK rows
 * of patch_id, C_prev: K x T) and keeps it with the context until the next call of it, the next cnmfe_fit_ring_model_ssub or the next upload;
 * the other two then read it:  Ybg(patch, t) = Bf(:, t) + b0_new  and  RSS = sum((Y(patch,:) - A*C - Ybg).^2)  (A: d x K CSC on the patch rows). */
int cnmfe_background_ssub(cnmfe_ctx *ctx, int patch_id, int fit_patch, int32_t ssub, int32_t K, const int64_t *A_colptr,
                          const int32_t *A_rowidx, const float *A_val, const float *C, int c_order, const float *b0_block /* d_b */);
int cnmfe_reconstruct_background_ssub(cnmfe_ctx *ctx, int patch_id, const float *b0_new /* d */, int64_t frame0, int64_t nframes,
                                       float *Ybg_out /* d x nframes, frame-major */, int out_memspace);
int cnmfe_compute_rss_ssub(cnmfe_ctx *ctx, int patch_id, int32_t K, const int64_t *A_colptr, const int32_t *A_rowidx,
                           const float *A_val, const float *C, int c_order, const float *b0_new /* d */, double *rss_out);

/* ---- (i) dF/F: [C_df, C_raw_df, Df] = extract_DF_F_endoscope(obj, Ybg)   @Sources2D/Sources2D.m:540-570, CNMFSetParms.m:73-74 (df_prctile 50, df_window [])
 *   Yf = (A ./ sum(A.^2, 1))' * Ybg  (:545);  Df = median(Yf, 2) / prctile(Yf, df_prctile, 2) without a window (:549-553), medfilt1(Yf, w, [], 2, 'truncate') /
 *   running_percentile(Yf(k, :), w, df_prctile) with one (:559, :563; utilities/running_percentile.m:74-121);  C_df = C ./ Df,  C_raw_df = C_raw ./ Df  (:554-555, :567-568).
 * Ybg = reconstruct_background() never exists as a whole: Yf is accumulated in a K x T fp64 matrix of the context, patch by patch and frame chunk by frame chunk.
 *   cnmfe_df_begin(ctx, K, T)                 the accumulator, zeroed.  64 <= T <= 147456, K = 0 is legal; CNMFE_ESTATE while one is open.
 *   cnmfe_df_add_frames(...)                  acc[ind_m[j], frame0 + t] += sum_i A(i, j) Ybg(i, t), t in [0, nframes): Ybg d x nframes frame-major fp32 in host or device
 *                                             memory (what cnmfe_reconstruct_background writes), A d x Km CSC over those d rows (empty columns are legal), ind_m the
 *                                             Km distinct accumulator rows.  The product of two fp32 values is formed and summed in fp64, in a fixed order.
 *   cnmfe_df_add_background[_ssub](...)       the same for all T frames of one patch with Ybg taken from the patch exactly as cnmfe_reconstruct_background[_ssub] takes
 *                                             it (same arguments, same preconditions: CNMFE_ESTATE without the residual / without cnmfe_background_ssub; a recorded or
 *                                             pending residual is realised first); A over the PATCH rows.  Frame chunks (a multiple of 4 frames, at most 256 MB of
 *                                             scratch kept with the patch's lane) are reconstructed and projected in turn: nothing of d x T is allocated.  Runs on the
 *                                             patch's lane; the projections of different lanes follow each other in call order, so the bits do not depend on the lanes.
 *   cnmfe_df_fetch / cnmfe_df_load            the accumulator to / from the host, K x T ROW-MAJOR doubles (a sharded run: fetch, all-reduce, load -- one K x T collective
 *                                             per session); load opens an accumulator if none is open.  cnmfe_df_dims: its K x T (CNMFE_ESTATE if none is open).
 *   cnmfe_df_finish(...)                      scales row k by inv_norm[k] = 1 / sum(A(:, k).^2) (K doubles, computed by the host in float64), takes the baseline, divides,
 *                                             writes the host outputs (ROW-MAJOR; each may be NULL) and closes the accumulator.  df_window = 0 or > T: no window, Df_out
 *                                             receives K doubles; else K x T doubles.  0 < df_window <= 16384 (DF_WINDOW_MAX: a longer window that is not longer than the
 *                                             recording is CNMFE_EUNSUPPORTED -- every output sample selects over its whole window); df_prctile outside [0, 100] or
 *                                             df_window < 0 is CNMFE_EINVAL.  (C, c_src) and (C_raw, raw_src) are trace SOURCES of section (h): a host pointer with its
 *                                             order (counted by merge_trace_uploads), CNMFE_BOUND or CNMFE_RES_CRAW.  Yf_out (may be NULL): the scaled K x T projection.
 *                                             With every output NULL the accumulator is only closed (what a caller does whose own session failed half way).
 * Deviations: a row of Yf that holds any non-finite value (a neuron with an empty footprint: 0 * Inf) gives NaN throughout its Df row (the reference's three
 * estimators disagree with each other on NaN); Df is float64, C_df and C_raw_df are float32, each (float)((double)C / Df).
 * medfilt1 and prctile are MathWorks functions, restated from their documentation (PARITY UNPINNED); running_percentile is in the reference tree.
 * Traces of up to 20346 frames (windowed: 20480) are staged in LDS by the baseline kernels, longer ones are read where they lie (option trace_long = 1 forces that: equal bits).
 * Every index is checked on the host before anything is launched: CNMFE_EINVAL for a row of A outside [0, d), an ind_m outside [0, K) or repeated, frames beyond T. */
int cnmfe_df_begin(cnmfe_ctx *ctx, int32_t K, int64_t T);
int cnmfe_df_add_frames(cnmfe_ctx *ctx, int64_t d, int64_t frame0, int64_t nframes, const float *Ybg /* d x nframes */, int memspace, int32_t Km,
                        const int64_t *A_colptr, const int32_t *A_rowidx /* in [0, d) */, const float *A_val, const int32_t *ind_m /* Km */);
int cnmfe_df_add_background(cnmfe_ctx *ctx, int patch_id, const float *b0_block /* d_b */, const float *b0_new /* d */, int32_t Km, const int64_t *A_colptr,
                            const int32_t *A_rowidx, const float *A_val, const int32_t *ind_m);
int cnmfe_df_add_background_ssub(cnmfe_ctx *ctx, int patch_id, const float *b0_new /* d */, int32_t Km, const int64_t *A_colptr, const int32_t *A_rowidx,
                                 const float *A_val, const int32_t *ind_m);
int cnmfe_df_dims(cnmfe_ctx *ctx, int32_t *K, int64_t *T);
int cnmfe_df_fetch(cnmfe_ctx *ctx, double *Yf_out /* K x T */);
int cnmfe_df_load(cnmfe_ctx *ctx, int32_t K, int64_t T, const double *Yf /* K x T */);
int cnmfe_df_finish(cnmfe_ctx *ctx, const double *inv_norm /* K */, double df_prctile, int64_t df_window /* 0: none */, const float *C, int c_src,
                    const float *C_raw, int raw_src, float *C_df_out /* K x T */, float *C_raw_df_out /* K x T */, double *Df_out /* K, or K x T with a window */,
                    double *Yf_out /* K x T or NULL */);

/* ---- (f) closing calls: the six panels of show_demixed_video   @Sources2D/show_demixed_video.m:70-81,94-127, demos/demo_large_data_1p.m:229
 * The displayed frames t_j = frame0 + j * stride (0-based, j < nframes, stride = kt >= 1) of one patch, every panel nframes x d frame-major over the patch's d pixels:
 *   raw       fp32   Y(p, t) = Yc + Ymean of the resident video
 *   bg        fp32   Ybg(p, t): the bits cnmfe_reconstruct_background[_ssub] writes for that frame (same arguments b0_block / b0_new, same preconditions: CNMFE_ESTATE
 *                    without the residual of (A_prev, C_prev) / without cnmfe_background_ssub; with bg_ssub > 1 the contiguous frames a run of displayed frames spans are
 *                    reconstructed into the lane's chunk scratch -- at most 256 MB, as for dF/F -- and read from there)
 *   signal    fp32   raw - bg, one fp32 subtraction (:107)
 *   denoised  fp32   (float) sum_k (double)A(p, k) (double)CC(k, t) over the pixel's stored neurons in ascending column order, an fp64 fma chain (:113)
 *   residual  fp32   (float)((double)raw - (double)bg - that fp64 sum) (:120)
 *   mixed     uint16 THREE planes of nframes x d (colour m at mixed_out + m * nframes * d): uint16(mix_scale * sum_k A(p, k) (col(k, m) CC(k, t))) in fp64 (:79-81) with
 *                    MATLAB's conversion -- round half away from zero, saturate to [0, 65535], NaN -> 0; mix_scale = 2 / amp_ac * 65536
 * A: d x Ksel CSC over the PATCH rows (empty columns are legal).  The traces are a trace SOURCE of section (h): a host matrix Ksel x T with its order (ind ignored; one
 * counted upload), or CNMFE_BOUND / CNMFE_RES_CRAW with ind[Ksel] = the rows of the call's neurons in the bound matrix.  col: Ksel x 3 floats, row-major.
 * Every output may be NULL and lies in host or device memory (out_memspace).  One thread per (pixel, frame), plain stores, no atomics, fixed summation order: two calls on
 * equal inputs are bit-identical, with any number of lanes.  nframes = 0 and Ksel = 0 are legal (Ksel = 0: denoised and mixed are zero).
 * CNMFE_EINVAL: stride < 1, nframes < 0 or > 65535, a displayed frame outside [0, T), a row of A outside [0, d), an ind outside the bound matrix, any other source. */
int cnmfe_demix_frames(cnmfe_ctx *ctx, int patch_id, const float *b0_block /* d_b */, const float *b0_new /* d */, int32_t Ksel, const int64_t *A_colptr,
                       const int32_t *A_rowidx, const float *A_val, const float *CC, int c_src, const int32_t *ind /* Ksel or NULL */, const float *col /* Ksel x 3 */,
                       double mix_scale, int64_t frame0, int64_t stride, int64_t nframes, float *raw_out, float *bg_out, float *signal_out, float *denoised_out,
                       float *residual_out, uint16_t *mixed_out /* 3 x nframes x d */, int out_memspace);
int cnmfe_demix_frames_ssub(cnmfe_ctx *ctx, int patch_id, const float *b0_new /* d */, int32_t Ksel, const int64_t *A_colptr, const int32_t *A_rowidx, const float *A_val,
                            const float *CC, int c_src, const int32_t *ind, const float *col, double mix_scale, int64_t frame0, int64_t stride, int64_t nframes,
                            float *raw_out, float *bg_out, float *signal_out, float *denoised_out, float *residual_out, uint16_t *mixed_out, int out_memspace);

/* ---- S6: post_process_spatial (connected = true, circular = false)
 * @Sources2D/post_process_spatial.m:19-32 -> endoscope/connectivity_constraint.m:1-18.
 * A is the whole-FOV d1*d2 x K CSC; keep[nnz] receives 1 for entries that survive. */
int cnmfe_post_process_spatial(cnmfe_ctx *ctx, int32_t d1, int32_t d2, int32_t K,
                               const int64_t *A_colptr, const int32_t *A_rowidx, const float *A_val,
                               uint8_t *keep);

/* ---- footprint image operations: compactSpatial / spatial_constraints.circular, search_method = 'dilate', trimSpatial
 * Small morphological operations on one footprint's bounding box, one workgroup per neuron, the box in LDS (cnmf_e_amd/csrc/footprint_ops.hpp).  A is the
 * whole-FOV d1*d2 x K CSC (rows ascending inside a column, inside [0, d1*d2): CNMFE_EINVAL otherwise), non-negative like every footprint; the calls run in the
 * context's global scope like cnmfe_post_process_spatial.
 * Arithmetic: everything that decides -- a comparison, the first maximum, a sum that is compared -- is fp64 on the fp32 values of A, each product and sum
 * rounded on its own (no fused multiply-add), in the order of the NumPy statements in cnmf_e_amd/hostops.py, whose results these calls EQUAL.  The cumulative
 * sum of the energy threshold is sequential, in the order of MATLAB's stable sort (squared value, then column-major pixel).  The first maximum is the first in
 * column-major order.  Iterations (component labels) are bounded by the cells of the box.  No atomics: two calls give the same bits.
 * Boxes: box[4 k ..] = (r0, c0, h, w), 0-based, of the non-zeros of column k grown by what the operation can reach and clipped to the field of view; off[k] = the
 * cells of the boxes in front of it, off[K] = all of them.  The result of column k lies at out + off[k], column-major over its box.  A box of more than 4096 cells
 * (64 x 64; with strel('disk', 4, 0): a 52 x 52 footprint, or a 10-pixel-wide dendrite 174 pixels long) is not computed: h = w = 0, host_col[k] = 1, and the caller
 * computes THAT column (the Python engine: with hostops); the read-only counter image_ops_host_columns (cnmfe_get_option) says how many columns of the last call
 * that was.  out = NULL: box, off and host_col only -- how a caller sizes out (out_cap cells; too small: CNMFE_EINVAL).  box, off, host_col are host memory; out
 * (keep) is host or device memory (out_memspace).
 *
 * cnmfe_circular_constraints: endoscope/circular_constraints.m:8-55 per column (Sources2D.compactSpatial, post_process_spatial.m:28-30).  The box is the bounding
 *   box of the non-zeros, whose edges are the image's edges for gradient(), the dilation and medfilt2 (the reference recurses on the crop).  out: the new values of
 *   the box (the support may grow inside it); an empty column has no cells, a box under 2 x 2 comes back unchanged.
 * cnmfe_search_dilate: utilities/threshold_components.m:20-62 + determine_search_location.m:89-98: medfilt2, the pixels holding nrgthr (in (0, 1]) of the energy,
 *   imclose by the 3 x 3 square (the dilation sees false outside the FOV, the erosion true), the 8-connected component with the most energy of the filtered
 *   image, imdilate by se (se_h x se_w bytes, row-major, origin at the centre) clipped at the FOV.  The last nb columns are dilated from > 0 without thresholding.
 *   out: one byte per cell, 1 = in the index set.  An se with an even side or a side above 15 leaves every non-empty column to the caller.
 * cnmfe_trim_spatial: @Sources2D/Sources2D.m:942-965: imopen by the sz x sz square (sz odd, 1 .. 9: CNMFE_EINVAL otherwise; erosion pads with +Inf, dilation with
 *   -Inf), temp = ai_open > max(ai) * thr (thr >= 0), 4-connected labels, keep[e] = 1 where l == l(argmax ai_open) -- all of the column when the opening removed
 *   everything --, ind_small[k] = sum(ai > 0) < min_pixel afterwards.  keep has one byte per stored entry like cnmfe_post_process_spatial's. */
int cnmfe_circular_constraints(cnmfe_ctx *ctx, int32_t d1, int32_t d2, int32_t K, const int64_t *A_colptr, const int32_t *A_rowidx, const float *A_val,
                               int32_t *box /* 4 K */, int64_t *off /* K + 1 */, float *out, int64_t out_cap, uint8_t *host_col /* K */, int out_memspace);
int cnmfe_search_dilate(cnmfe_ctx *ctx, int32_t d1, int32_t d2, int32_t K, const int64_t *A_colptr, const int32_t *A_rowidx, const float *A_val,
                        const uint8_t *se, int32_t se_h, int32_t se_w, int32_t nb, double nrgthr,
                        int32_t *box /* 4 K */, int64_t *off /* K + 1 */, uint8_t *out, int64_t out_cap, uint8_t *host_col /* K */, int out_memspace);
int cnmfe_trim_spatial(cnmfe_ctx *ctx, int32_t d1, int32_t d2, int32_t K, const int64_t *A_colptr, const int32_t *A_rowidx, const float *A_val,
                       double thr, int32_t sz, int32_t min_pixel, uint8_t *keep /* nnz */, uint8_t *ind_small /* K */, uint8_t *host_col /* K */, int out_memspace);

/* ---- measurement: per-kernel HIP-event timing on the engine's stream ---------
 * on = 1: every launch is bracketed by a pair of events; on = 2: only the kernels a roofline is quoted for (residual sweep, ring solve, window
 * projection / table correction, the two residual projections) -- the pairs cost host and device time per launch, which a run that wants its
 * wall time undisturbed avoids; on = 0: off. */
int cnmfe_profile_enable(cnmfe_ctx *ctx, int on);
int cnmfe_profile_reset(cnmfe_ctx *ctx);
/* number of distinct kernel names seen; name/total_ms/calls of the i-th */
int cnmfe_profile_count(cnmfe_ctx *ctx);
int cnmfe_profile_get(cnmfe_ctx *ctx, int i, char *name, int name_cap, double *total_ms, int64_t *calls);
int cnmfe_synchronize(cnmfe_ctx *ctx);
/* Tunables; unknown names -> CNMFE_EINVAL.  Thirteen behaviour switches, every default = the measured path, every other value parity-tested against it:
 *   r1_variant        R1 sweep kernel (14: duo-role LDS-DMA kernel, the default where it applies; -1: the generic kernel)
 *   r1_delta, r1_lazy, r1_defer    incremental residual (see cnmfe_residual): fold a footprint-term difference into the resident Ysig / only record a request nobody
 *                     reads / sweep without the term and keep it pending.  Default 1 each.
 *   r1_virtual        default 1: a cnmfe_residual without an output buffer records its request and the two updates project the centred video instead of a swept
 *                     Ysig; 0 restores the sweep
 *                     How the four combine (one rule for cnmfe_residual and cnmfe_residual_ssub, cnmf_e_amd/csrc/residual_plan.hpp): while a residual of the same call
 *                     is kept for the patch (swept or recorded) and r1_delta is on, a request only adds its footprint term -- pending with r1_lazy and no output
 *                     buffer, folded in at once otherwise.  Else a request without an output buffer is recorded when r1_virtual, r1_lazy and r1_delta are all on
 *                     (its term pends: recording needs the other two).  Else the sweep runs; r1_defer needs r1_lazy as well.  r1_delta = 0 therefore sweeps on
 *                     every request.  r1_variant: any value other than -1, 10, 11, 14 means 14; 14 serves radius 15 without a footprint term inside the sweep (11
 *                     takes over with one), 11 radius 15, 10 radius 15 / 18 and the low-resolution radii 5, 6, 8, 9 (where it is the only specialised kernel);
 *                     a ring that is not the full ring of its radius, or any other radius, runs the generic kernel
 *   ssub_virtual      the same for cnmfe_residual_ssub (through the resampling maps): 2 always, 1 (default) on patches of at least 5e8 samples -- below that the
 *                     low-resolution sweep is the faster form, profiles/r05/ssub_virtual_check.txt --, 0: the low-resolution sweep + upsample
 *   gram_incremental  default 1: the covariance table of the VIDEO is kept and corrected per fit (see cnmfe_fit_ring_model); 0: the direct Gram of Bf every fit
 *   proj_i8_planes    default 3: the temporal projection on the int8 pipe reads the upper three of the video's four digit planes (24-bit samples: 3/4 of the bytes;
 *                     A, C move by < 1e-7); 4: all of them
 *   solve_staged      default 1: the ring solve samples the footprints' U~ and A out of per-neuron windows (ring_solve_staged.hpp; bit-identical weights); 0: it walks
 *                     the CSR rows and slot tables
 *   solve_inv         default 0; 1: fits of a patch from its second one with footprints on solve their pixels out of explicit inverses of the VIDEO's normal equations
 *                     (built once in front of that fit, the bytes of solve_packed's systems once more; the footprints enter by the Woodbury identity, the ridge's
 *                     drift by a short series: ring_solve_inv.hpp); 2: built in front of the first such fit; 0: every fit factors every pixel's system
 *   solve_inv_terms   default 5: terms of the ridge series before a pixel is left to the factorising kernel and its inverse rebuilt
 *   solve_packed      default 1: the ring solve reads per-pixel packed copies of the video's normal equations (43 KB per patch pixel at 96 ring offsets, allocated
 *                     when that much + 8 GB is free) and applies the footprints' corrections in registers; 0: the block-pair table is swept and gathered from
 *   gram_i8           default 1: the table (and the direct Gram of the fallback) on the int8 matrix pipe from 32-bit fixed-point digit planes, exact int32
 *                     accumulation, up to 24576 used frames; 0: the fp64 matrix pipe
 *   win_i8            default 1: the digit planes stay resident (one more video's worth of memory, taken only when that leaves 8 GB free) and every fit's window
 *                     projection runs on the int8 pipe; 0: the fp64 kernel on the centred video
 *   win_i8_planes     default 0 = 3 when the sums run over at least 2048 frames, else 4 (3 / 4 force it): the fit's window projection (and the all-frames table of a strided recording) reads the upper three digit planes of the video -- 24-bit
 *                     samples, 3/4 of the bytes (1.93 -> 1.48 ms at 512 x 512 x 10000); W within 2e-6 of the float64 oracle's (observed 5e-7 .. 1.8e-6 of the largest
 *                     weight; with all four planes, win_i8_planes = 4: 4e-8 .. 2e-7), A and C unchanged at ~1e-7
 *   proj_tiled / proj_i8   default 1 / 1: the temporal projection on the int8 pipe out of a pixel-major copy of the digit planes (needs win_i8), else out of a copy of
 *                     the centred video in its own read order (one video's worth either, same rule); 0 / 0: the frame-major video on the fp64 pipe.  The tables over ALL frames
 *                     (spatial update, temporal projection) sum inside frame segments of at most 24576 frames, recordings up to 16 x 24576 frames
 *   lanes             default 1; 2 .. 4 (set BEFORE the first patch is created; until then a further call replaces the lanes, 1 drops them, the count in force does
 *                     nothing -- read-only counter lanes_live): the patches alternate between that many execution lanes -- a HIP stream + a set of the
 *                     context's scratch each -- so that the small kernels of independent patches overlap (update_*_parallel.m: parfor); calls on what the patches share
 *                     (bound traces, stitch, the temporal jobs' sweep, post-processing) join the lanes.  Results are bit-equal to lanes = 1 (tests/test_gpu_lanes.py)
 *   sweep_dag         default 1: the maxIter Gauss-Seidel sweeps of a HALS update (HALS_spatial.m:36-44, HALS_temporal.m:59-68, with or without the in-sweep
 *                     deconvolution) are launched level by level of ONE dependency graph over (sweep, neuron) items -- the same reads and writes per item, equal results,
 *                     fewer and fuller launches (512 x 512, K = 500: 21 instead of 25); 0: sweep after sweep, level by level (rounds 1-5)
 *   temporal_early    default 1: the hand-over from the spatial to the temporal update without device idle time -- the temporal projection is queued behind the
 *                     spatial update's connectivity kernel (cnmfe_temporal_early_project, below) and the Gauss-Seidel levels are queued without the host wait for
 *                     A'A (aa and its check are taken on the device; the wait stays when a footprint term over more than 512 traces was applied, whose list kernel
 *                     may overflow).  2: the projection only, 3: the levels only, 0: neither.  Results are bit-equal (tests/test_gpu_handover.py)
 *   fit_side          default 1: a ring fit that queues its window projection first (the video's table exists and A has entries: every fit of a patch but its first)
 *                     queues what follows up to k_win_fix and reads nothing the projection writes -- the trace sums and the K x K trace Gram, the CSR rows of A,
 *                     sum(A, 2), ind_active, b0, slot_of, the staged windows' metadata -- on a second stream of the context, forked in front of the projection and joined
 *                     in front of k_win_fix, so the GPU runs it underneath the projection.  2: the same streams, joined in front of the projection (nothing overlaps:
 *                     tests).  0: one stream.  Inert with lanes > 1.  Results are bit-equal (tests/test_gpu_fit_side.py)
 *   ring_side         default 1: a ring fit records an event right behind its solve and queues, on the context's side stream behind THAT event, what depends on the
 *                     new W alone -- the statistics the next fit asks for (ring_pmax and its downloads) and, when the fit has footprints, the W*A tables (the CSR
 *                     rows of A, r1_ring_wa, the error word) of the residual request that follows the fit, in buffers of their own -- so the GPU runs them beside
 *                     the spatial update's kernels.  The first cnmfe_residual request behind the fit that is only recorded (no output, no sweep) takes the tables
 *                     when its A is the fit's, entry for entry, and makes the compute stream wait for them first; any other request builds its own as before.
 *                     2: the same streams and code, the wait directly behind the fit's launches (nothing overlaps: tests).  0: one stream.  Inert with lanes > 1,
 *                     with more than one patch in the context, in a fit with thresh_outlier and for cnmfe_residual_ssub.  Results are bit-equal
 *                     (tests/test_gpu_trace_ahead.py)
 *   prealloc          default 1: cnmfe_fit_reserve may allocate the fit's large buffers ahead of the first fit
 *   bg_svd_tol_exp    default 12: cnmfe_bg_svd_fit stops when every wanted component's residual |M u_i - theta_i u_i| is at most 10^-value theta_1 (1 .. 16)
 *   bg_svd_max_iter   default 40: ... or after this many iterations (two reads of the video each); the fit then reports converged = 0
 * A deployment short of HBM sets win_i8 = proj_tiled = 0 (and solve_packed = 0) or leaves it to the engine, which falls back by itself.
 * Diagnostics (scripts/): solve_probe, r1_probe (phase probes: results are NOT the product's), deconv_trace, host_trace (1: host-side phase times of every call on
 * stderr, 2: + slow launch calls), debug (1: NaN-poison never-computed table entries), trace_long (default 0: the seed-statistics, peel-trace, trace-difference and
 * trace-tag kernels keep the trace in LDS while it fits beside the Welch transform, T <= 20416, and in global memory beyond; 1: the long flavour at every T --
 * results are bit-equal, tests/test_gpu_long_flavour.py; the dF/F baselines of section (i) follow the same option with their own limits of 20346 / 20480 frames, tests/test_gpu_dff.py).
 * Round 6 removed the retired names rounds 2-5 still accepted and ignored (gram_mode, gram_flush, solve_defer, solve_mode, solve_gfill, gram_kernel, r1_arc_d,
 * r1_arc_bias, r1_duo_ord) and the experiment switches tile_order, gram_probe, r1_nseg.
 * Every option can be preset for a process with CNMFE_OPTS="name=value,..." (logged once on stderr). */
int cnmfe_set_option(cnmfe_ctx *ctx, const char *name, int64_t value);
/* The value cnmfe_set_option (or CNMFE_OPTS) gave an option last; an option that was never set reports CNMFE_EINVAL (its default, above, holds).  Also the
 * read-only counters of the hand-over: temporal_early_hits / _drops (early projections a temporal update took / found but could not take), temporal_early_declined
 * (requests the projection could not serve), temporal_early_entries / temporal_proj_entries ((block, neuron) entries of the last early / of the last projection),
 * temporal_nowait (temporal updates whose levels were queued without the host wait), and merge_trace_uploads (K x T matrices the merge / tag entry points and
 * cnmfe_traces_load took from the host: 0 while they work on the context's own matrices), and bound_K / bound_T (the shape of the bound trace matrix, 0 without
 * one: what a gateway sizes the outputs of cnmfe_merge_apply with), and lanes_live (the execution lanes in force, 1 without option lanes), and image_ops_host_columns (columns the last footprint image operation left to the caller). */
int cnmfe_get_option(cnmfe_ctx *ctx, const char *name, int64_t *value);

/* The hand-over between the spatial and the temporal update (option temporal_early).  After cnmfe_update_spatial_fetch_connected[_async] of a patch that is the
 * whole field of view, cnmfe_temporal_early_project queues the temporal update's projection of the post-processed result where it lies on the device (IND: the
 * mask pattern of that spatial update) and returns a token, 0 when it declines.  A caller whose next cnmfe_hals_temporal passes EXACTLY that result -- the fetched
 * values where the keep flag is set, stored zeros dropped, every column non-empty -- says so with cnmfe_temporal_early_claim(token) right before the call; the
 * update then starts from the queued projection.  Unclaimed, or stale in any way (another K, patch, T, residual request, spatial update, projection option), the
 * early result is dropped and the update projects as before: the values are the same either way. */
int cnmfe_temporal_early_project(cnmfe_ctx *ctx, int32_t K, const int64_t *IND_colptr, const int32_t *IND_rowidx, int64_t *token);
int cnmfe_temporal_early_claim(cnmfe_ctx *ctx, int64_t token);

/* ---- background_model = 'svd': the low-rank background of a patch         update_background_parallel.m:238-242 -> endoscope/fit_svd_model.m, svdsecon.m
 * On the BLOCK (d_b x T):  Bf = (Y - mean(Y,2)) - A (C - mean(C,2));  [u,s,v] = the top nb singular triplets of Bf - mean(Bf,2);
 *   b = u(ind_patch,:) s,  f = v',  b0 = Ymean(ind_patch) - A(ind_patch,:) Cmean - b mean(f,2);   nb = 0: b = f = 0, b0 = Ymean(ind_patch) - A(ind_patch,:) Cmean.
 * The engine never forms Bf or a Gram matrix of it: block subspace iteration with a Rayleigh-Ritz step on 16 columns, two reads of the resident video per
 * iteration, every sum in fp64 and in a fixed order (two fits of the same input give the same bits; a bound C and the same C uploaded give the same bits).
 * Each u_i is scaled so that its entry of largest magnitude is positive.  thresh_outlier and sn play no part: the reference's outlier branch tests a misspelt
 * variable and never runs.
 *   cnmfe_bg_svd_fit      A: d_b x K CSC over BLOCK rows, C: K x T or (NULL, CNMFE_BOUND) / (rows, CNMFE_BOUND_ROWS).  K = 0 (or an empty A) is the reference's
 *                         A = ones, C = zeros branch.  The iteration stops when |M u_i - theta_i u_i| <= tol theta_1 for every i <= nb (M = Bf Bf', measured, not
 *                         estimated) or at the iteration cap: options bg_svd_tol_exp (tol = 10^-value, default 12) and bg_svd_max_iter (default 40).  A fit that
 *                         hits the cap is NOT an error: it keeps what it has and says so in cnmfe_bg_svd_stats.  CNMFE_EUNSUPPORTED for nb outside 0 .. 8 or
 *                         nb > min(d_b, T).  The factors stay with the patch on the device in fp64.
 *   cnmfe_bg_svd_get      b: d x nb (column-major: nb columns of d), f: nb x T (row-major), b0: d; any may be NULL.  CNMFE_ESTATE before a fit or a set.
 *   cnmfe_bg_svd_set      transplants a saved background (the same layouts; nb = 0: b and f are ignored).
 *   cnmfe_bg_svd_stats    out[20]: [0] reads of the video, [1] iterations, [2] converged (1 / 0), [3] nb, [4 .. 11] the residual of each component relative to
 *                         theta_1 as the last iteration measured it, [12 .. 19] the singular values.
 *   cnmfe_residual_lowrank  Ysig = Y(ind_patch,:) - (b f + b0) of the patch, computed in fp64 and rounded once to fp32, resident for cnmfe_update_spatial,
 *                         cnmfe_hals_temporal[_deconv / _job] and cnmfe_fast_temporal exactly as the residual of cnmfe_residual is (Ysig_out as there).  A fit, a set
 *                         and an upload of the video invalidate it: an update without it is CNMFE_ESTATE.  cnmfe_compute_rss, cnmfe_reconstruct_background and what
 *                         is built on them serve the ring model only (CNMFE_EUNSUPPORTED on this residual).
 *   cnmfe_peel_open_lowrank  the SECOND pass under this model (@Sources2D/initComponents_residual_parallel.m:107-122,195-199,224-227): the session on the PATCH and on
 *                         Yres = Y(patch) - A(patch, ind) C(ind, :) - (b f + b0).  With ssub = tsub = 1 the video is written in ONE pass from the centred video and
 *                         the fp64 factors (fp64 fma chain: b f over ascending i, then the pixel's footprints in ascending column order; one rounding to fp32; 16
 *                         bytes read and 16 written per pixel and frame quad): no Ysig is realised, no residual is required, and the patch's residual state is the
 *                         same before the open and after cnmfe_peel_close.  Arguments, outputs and refusals are those of cnmfe_peel_open_residual_ds (A over the
 *                         PATCH rows, no open session, no derived patch, the factors' ranges) except that no residual is asked for; CNMFE_ESTATE before a fit or a
 *                         set.  A failed open leaves no session.  With other factors Ysig is realised as cnmfe_residual_lowrank realises it and the session is
 *                         cnmfe_peel_open_residual_ds' on it: that residual goes with the session.  extract / apply / close are the session's as ever.
 *   cnmfe_demix_frames_lowrank  cnmfe_demix_frames under this model: bg = (float)(b0(p) + sum_i b(p, i) f(i, t)), an fp64 fma chain over ascending i; raw, signal,
 *                         denoised, residual and mixed keep their expressions on that bg.  No b0 argument, no residual read, requested or changed; CNMFE_ESTATE
 *                         before a fit or a set.
 *   cnmfe_init_temporal_lowrank  known footprints under this model (@Sources2D/initTemporal.m:180-192): the traces of the footprints A AND the temporal factors of
 *                         the patch's resident b on its resident video.  A: d_b x K CSC over BLOCK rows; the rows outside the PATCH are dropped (:103-109).  With
 *                         M = [A(patch, :), b] the call solves (M'M) X = M'(Y - mean(Y,2)) for all frames -- M'M and M'Y accumulated in fp64 in a fixed order, the
 *                         video read once per projection pass (counter init_temporal_lowrank_video_reads: 1 unless a 16 x 16 block meets more than 64 columns),
 *                         M'M Cholesky-factored on the host in float64, the two triangular solves on the device in fp64 -- and then runs HALS_temporal's sweeps
 *                         from C = X(1:K, :) on Y - (b f + b0): iters_plain plain sweeps and iters_last more (with opts: the in-sweep AR(1) FOOPSI, kernel
 *                         parameters estimated fresh), as cnmfe_init_temporal does.  Outputs as there (C, C_raw, S, kernel_pars, sn, AA: any may be NULL; C_raw and
 *                         AA stay on the device for cnmfe_stitch_add) plus f_out (nb x T, row-major) and b0_out (d), float64, either may be NULL.  Afterwards the
 *                         patch's f is X(K+1:end, :), its b0 the pixel mean of the patch, b is unchanged, and the patch is in the state cnmfe_bg_svd_set leaves:
 *                         a resident Ysig is invalid.  A column of b that is identically zero is left out of the system; its row of f is 0 (the reference
 *                         divides by a singular matrix).  CNMFE_ESTATE before a fit or a set, and when a Cholesky pivot is <= n eps max(diag M'M) (the message
 *                         names the patch and the pivot); CNMFE_EUNSUPPORTED for more than 2048 unknowns (option init_temporal_lowrank_nmax lowers the cap), for
 *                         a derived patch and for deconvolution other than 'ar1' / 'foopsi'.  A failed call changes nothing of the patch.  Two calls give the
 *                         same bits.  Counter init_temporal_lowrank_factor_us: the host factorisation's time of the last call. */
int cnmfe_init_temporal_lowrank(cnmfe_ctx *ctx, int patch_id, int32_t K, const int64_t *A_colptr, const int32_t *A_rowidx /* BLOCK rows */, const float *A_val,
                                int32_t iters_plain, int32_t iters_last, const cnmfe_deconv_opts *opts, float *C_out, float *C_raw_out, float *S_out,
                                float *kernel_pars_out, float *sn_out, float *AA_out, double *f_out, double *b0_out, int c_order);
int cnmfe_bg_svd_fit(cnmfe_ctx *ctx, int patch_id, int32_t nb, int32_t K, const int64_t *A_colptr, const int32_t *A_rowidx /* BLOCK rows */, const float *A_val,
                     const float *C, int c_order);
int cnmfe_bg_svd_get(cnmfe_ctx *ctx, int patch_id, double *b, double *f, double *b0);
int cnmfe_bg_svd_set(cnmfe_ctx *ctx, int patch_id, int32_t nb, const double *b, const double *f, const double *b0);
int cnmfe_bg_svd_stats(cnmfe_ctx *ctx, int patch_id, double out[20]);
int cnmfe_residual_lowrank(cnmfe_ctx *ctx, int patch_id, float *Ysig_out, int out_memspace);
int cnmfe_peel_open_lowrank(cnmfe_ctx *ctx, int patch_id, int32_t ssub, int32_t tsub, int32_t Ksel, const int64_t *A_colptr, const int32_t *A_rowidx /* in [0, d) */,
                            const float *A_val, const float *C, int c_order, const float *psf, int32_t psf_n, float sig, float *Cn_out /* d1s * d2s */,
                            float *PNR_out /* d1s * d2s */, float *Sn_out /* d1s * d2s or NULL */, float *Y_out /* d1s * d2s x Ts or NULL */, int out_memspace);
int cnmfe_demix_frames_lowrank(cnmfe_ctx *ctx, int patch_id, int32_t Ksel, const int64_t *A_colptr, const int32_t *A_rowidx, const float *A_val, const float *CC,
                               int c_src, const int32_t *ind /* Ksel or NULL */, const float *col /* Ksel x 3 */, double mix_scale, int64_t frame0, int64_t stride,
                               int64_t nframes, float *raw_out, float *bg_out, float *signal_out, float *denoised_out, float *residual_out,
                               uint16_t *mixed_out /* 3 x nframes x d */, int out_memspace);

#ifdef __cplusplus
}
#endif
#endif /* CNMFE_H */
