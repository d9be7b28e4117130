// Shared internals of the CNMF-E HIP engine (gfx950 only).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include <stdarg.h>
#include <string.h>
#include <string>
#include <vector>
#include <cstring>
#include <chrono>
#include <cmath>
#include <map>
#include <algorithm>
#include "../../include/cnmfe.h"
#include "ring_plan.hpp"
#include "residual_plan.hpp"
#include "kept_results.hpp"

namespace cnmfe {

// a 16-byte load of data that is read ONCE per pass (the digit planes of the video in k_win_proj_i8): non-temporal, so the stream does not evict the trace planes every
// workgroup re-reads (1.97 -> 1.94 ms at H, three runs each on one lease; the fp32 stream of k_vp_proj_b showed no difference and keeps plain loads)
typedef unsigned nt_u32x4_t __attribute__((ext_vector_type(4)));
__device__ __forceinline__ uint4 ld_stream(const uint4 *p) {
    const nt_u32x4_t v = __builtin_nontemporal_load(reinterpret_cast<const nt_u32x4_t *>(p));
    return make_uint4(v.x, v.y, v.z, v.w);
}


extern thread_local char g_err[1024];
inline int fail(int code, const char *fmt, ...) {
    va_list ap; va_start(ap, fmt); vsnprintf(g_err, sizeof(g_err), fmt, ap); va_end(ap);
    return code;
}

#define CK(call) do { hipError_t e_ = (call); if (e_ != hipSuccess) \
    return cnmfe::fail(CNMFE_EHIP, "%s:%d %s -> %s", __FILE__, __LINE__, #call, hipGetErrorString(e_)); } while (0)
#define RET(x) do { int r_ = (x); if (r_ != 0) return r_; } while (0)

void pin_flush_all();         // api.hip: enqueue the small uploads every context still holds back (see cnmfe_ctx::st)
void pin_flush_range(const void *p, size_t bytes);   // ... those into [p, p + bytes) -- before that device memory is freed (only its owner's context holds any)

// ---- owned device buffer -----------------------------------------------------
struct DevBuf {
    void *p = nullptr; size_t cap = 0;
    ~DevBuf() { if (p) { pin_flush_range(p, cap); (void)hipFree(p); } }
    DevBuf() = default;
    DevBuf(const DevBuf &) = delete; DevBuf &operator=(const DevBuf &) = delete;
    // a move steals the allocation and leaves the source empty; what the target held is released first (nothing, wherever two buffers change places)
    DevBuf(DevBuf &&o) noexcept : p(o.p), cap(o.cap) { o.p = nullptr; o.cap = 0; }
    DevBuf &operator=(DevBuf &&o) noexcept {
        if (this != &o) { if (p) { pin_flush_range(p, cap); (void)hipFree(p); } p = o.p; cap = o.cap; o.p = nullptr; o.cap = 0; }
        return *this;
    }
    int ensure(size_t bytes) {
        if (bytes <= cap) return 0;
        // a buffer that GROWS gets half as much again: index lists and value arrays follow nnz(A) / nnz(IND), which creep up over the first iterations, and every
        // hipFree drains the device -- 0.8-0.9 ms of the host blocked inside an upload while the fit's kernels ran (host_trace, one rank's share of c4)
        const size_t grown = (p && bytes < (size_t(64) << 20)) ? std::max(bytes, cap + cap / 2) : bytes;       // (small buffers only: a table or a video that grows is not over-allocated)
        static const bool trace_alloc_ = getenv("CNMFE_TRACE_ALLOC") != nullptr;          // (diagnostic: every re-allocation of a grown buffer on stderr -- hipFree drains the device)
        if (trace_alloc_ && p) fprintf(stderr, "[alloc] grow %zu -> %zu bytes (hipFree + hipMalloc)\n", cap, grown);
        if (p) { pin_flush_range(p, cap); (void)hipFree(p); p = nullptr; cap = 0; }     // (an upload into the old allocation may still be held back)
        size_t want = (grown + 255) & ~size_t(255);
        hipError_t e = hipMalloc(&p, want);
        if (e != hipSuccess) { p = nullptr; return fail(CNMFE_ENOMEM, "hipMalloc(%zu) failed: %s", want, hipGetErrorString(e)); }
        cap = want; return 0;
    }
    // for buffers that change hands (swap) between the context's scratch and the patches: every one of them grows to the largest request seen (`hw`),
    // otherwise a buffer sized for one patch's traces is re-allocated -- hipFree drains the device -- whenever it lands under a patch with more
    int ensure_hw(size_t bytes, size_t &hw) { if (bytes > hw) hw = bytes; return ensure(hw); }
    template <class T> T *as() const { return reinterpret_cast<T *>(p); }
    void swap(DevBuf &o) { std::swap(p, o.p); std::swap(cap, o.cap); }
};

// ---- per-kernel event timing ---------------------------------------------------
struct Profiler {
    int on = 0;                        // 0 off, 1 every kernel, 2 only the kernels a roofline is quoted for (a pair of events costs a few microseconds of
                                       // host AND device time per launch: thousands of small launches per iteration feel it, cnmfe_profile_enable)
    static bool selected(const char *n) {
        static const char *const sel[] = {"residual_r1", "bg_ring_solve", "bg_win_proj", "bg_cov_correct", "spatial_proj_U", "temporal_proj_U"};
        for (const char *s : sel) if (!strcmp(n, s)) return true;
        return false;
    }
    bool want(const char *n) const { return on == 1 || (on == 2 && selected(n)); }
    struct Rec { hipEvent_t a, b; int id; };
    std::vector<std::string> names;
    std::vector<double> total_ms; std::vector<int64_t> calls;
    std::vector<Rec> pending;
    std::vector<hipEvent_t> pool;
    int id_of(const char *n) {
        for (size_t i = 0; i < names.size(); ++i) if (names[i] == n) return (int)i;
        names.push_back(n); total_ms.push_back(0); calls.push_back(0); return (int)names.size() - 1;
    }
    hipEvent_t ev() { if (!pool.empty()) { hipEvent_t e = pool.back(); pool.pop_back(); return e; }
                      hipEvent_t e; (void)hipEventCreate(&e); return e; }
    void begin(const char *n, hipStream_t s, Rec &r) { r.id = id_of(n); r.a = ev(); r.b = ev(); (void)hipEventRecord(r.a, s); }
    void end(hipStream_t s, Rec &r) { (void)hipEventRecord(r.b, s); pending.push_back(r); }
    void drain() {
        for (auto &r : pending) {
            (void)hipEventSynchronize(r.b); float ms = 0; (void)hipEventElapsedTime(&ms, r.a, r.b);
            total_ms[r.id] += ms; calls[r.id] += 1; pool.push_back(r.a); pool.push_back(r.b);
        }
        pending.clear();
    }
    void reset() { drain(); for (auto &t : total_ms) t = 0; for (auto &c : calls) c = 0; }
    ~Profiler() { drain(); for (auto e : pool) (void)hipEventDestroy(e); }
};

// launch wrapper: LAUNCH(ctx, "name", kernel, grid, block, shmem, args...)
#define LAUNCH(ctx, name, kern, grid, block, shmem, ...) do { \
    cnmfe::Profiler::Rec pr_; bool pon_ = (ctx)->prof.on && (ctx)->prof.want(name); \
    const bool ltr_ = (ctx)->trace_level >= 2; \
    const auto lt0_ = ltr_ ? std::chrono::steady_clock::now() : std::chrono::steady_clock::time_point(); \
    hipStream_t lst_ = (ctx)->st(); \
    if (pon_) (ctx)->prof.begin(name, lst_, pr_); \
    const auto lt1_ = ltr_ ? std::chrono::steady_clock::now() : std::chrono::steady_clock::time_point(); \
    hipLaunchKernelGGL(kern, grid, block, shmem, lst_, __VA_ARGS__); \
    if (ltr_) { const auto lt2_ = std::chrono::steady_clock::now(); const double la_ = std::chrono::duration<double, std::milli>(lt1_ - lt0_).count(), lb_ = std::chrono::duration<double, std::milli>(lt2_ - lt1_).count(); \
        if (la_ + lb_ > 2.0) fprintf(stderr, "[host_trace] launch %s: flush of held-back uploads %.2f ms, launch call %.2f ms\n", name, la_, lb_); } \
    if (pon_) (ctx)->prof.end(lst_, pr_); \
    hipError_t le_ = hipGetLastError(); \
    if (le_ != hipSuccess) return cnmfe::fail(CNMFE_EHIP, "launch %s failed: %s", name, hipGetErrorString(le_)); \
} while (0)

constexpr int PMAX_RING = 128;    // max ring neighbours supported (r=18 -> 120)
constexpr int BLK = 16;           // 16x16-pixel covariance blocks
constexpr int BLKPX = BLK * BLK;

// ---- sparse helpers (host) ------------------------------------------------------
struct HostCSR { std::vector<int32_t> rowptr;   /* nnz < 2^31 everywhere (checked by the callers): the device wants 32-bit row pointers anyway */ std::vector<int32_t> col; std::vector<float> val; std::vector<int32_t> src; };
// CSC (ncol columns, nrow rows) -> CSR with `src` = index into the CSC arrays
inline void csc_to_csr(int64_t nrow, int32_t ncol, const int64_t *colptr, const int32_t *rowidx, const float *val, HostCSR &out) {
    int64_t nnz = colptr[ncol];
    out.rowptr.assign(nrow + 1, 0); out.col.resize(nnz); out.val.resize(nnz); out.src.resize(nnz);
    for (int64_t e = 0; e < nnz; ++e) out.rowptr[rowidx[e] + 1]++;
    for (int64_t r = 0; r < nrow; ++r) out.rowptr[r + 1] += out.rowptr[r];
    std::vector<int32_t> cur(out.rowptr.begin(), out.rowptr.end() - 1);
    for (int32_t k = 0; k < ncol; ++k)
        for (int64_t e = colptr[k]; e < colptr[k + 1]; ++e) {
            int32_t pos = cur[rowidx[e]]++; out.col[pos] = k; out.val[pos] = val ? val[e] : 1.0f; out.src[pos] = (int32_t)e;
        }
}

// the longest trace the Welch estimator takes: pwelch's segment length floor(T / 4.5) <= 32768 = the largest transform built (two 16384-point halves in LDS)
constexpr int WELCH_TMAX = 147456;

// a greedy-initialisation session of one patch (peel.hpp, cnmfe_peel_open .. cnmfe_peel_close): the filtered block HY, the working copy Yw of the video (both
// [ceil(n / 4)][d_b] float4), GetSn of HY per block pixel (fp64), the detrend basis, ci | y_bg (fp64, n each) and the box kernels' scratch
// The session runs on the geometry of its SOURCE video: the centred block (cnmfe_peel_open: d = d_b, nr_b x nc_b, y_bg adds the pixel mean back) or the
// residual video of the patch (cnmfe_peel_open_residual: Yw starts as Yres = Ysig - A C, d x nr x nc of the patch, no pixel mean -- the residual carries its own)
// or the down-sampled block (cnmfe_peel_open_ds, ds.hpp: Yw starts as dsData of the block on the ceil(nr_b / ssub) x ceil(nc_b / ssub) grid with floor(n / tsub)
// frames; y_bg adds the session's OWN pixel mean box(ymean) -- own_mean -- or none behind a pre-detrend -- no_mean).  keep_resid: a residual session that never
// read P->ysig (cnmfe_peel_open_lowrank at full resolution): closing it leaves the patch's residual state as it is
struct PeelSession { DevBuf hy, yw, sn, q, ci, scr, ymean; int64_t n = 0, nq = 0; int M = 0; int64_t d = 0; int nr = 0, nc = 0; bool residual = false, own_mean = false, no_mean = false, keep_resid = false; };
// the video a seed / peel pass reads: [ceil(n / 4)][d] float4, nr x nc pixels column-major
struct SeedSrc { const float4 *y4; int64_t d; int nr, nc; };

// ---- the residual of a patch: what lies beside Ysig (the rules that move it: residual_plan.hpp; DESIGN.md, "Residual state") ------
// The footprint term (W A)(C - mean C) as kept beside Ysig: ELL rows of W A per patch pixel (cnt | k | v), the centred traces (cc, K rows of stride ldc) and the
// means they were centred about (cm, fp64).  ac: the term has footprints at all (else the buffers are not read).
struct FootTerm {
    bool ac = false; int64_t ldc = 0; int32_t K = 0;
    DevBuf cnt, k, v, cc, cm;
    void set(bool ac_, int64_t ldc_, int32_t K_) { ac = ac_; ldc = ldc_; K = K_; }
    // the term a call has just built in the context's scratch moves here, what lay here goes back as scratch: buffers change hands, none is allocated or freed
    void take(bool ac_, int64_t ldc_, int32_t K_, DevBuf &cnt_, DevBuf &k_, DevBuf &v_, DevBuf &cc_, DevBuf &cm_) {
        set(ac_, ldc_, K_);
        if (ac_) { cnt.swap(cnt_); k.swap(k_); v.swap(v_); cc.swap(cc_); cm.swap(cm_); }
    }
    void swap(FootTerm &o) { std::swap(ac, o.ac); std::swap(ldc, o.ldc); std::swap(K, o.K); cnt.swap(o.cnt); k.swap(o.k); v.swap(o.v); cc.swap(o.cc); cm.swap(o.cm); }
    rplan::TermView view() const { return {ac, ldc, K}; }
};
// Ysig of a patch is in one of three forms.  NONE: nothing valid (the video, W or b0 changed: invalidate()).  VIRTUAL: a request is recorded and no sweep has run --
// the two updates take Ysig C' and A' Ysig from the centred video (vproj.hip), whoever reads Ysig itself calls residual_realize first.  RESIDENT: Patch::ysig holds
// Ysig with the `applied` term in it.  In both valid forms a further term may be `pending`: the residual the caller asked for is Ysig - applied + pending; the updates
// add that difference through their projections (residual_term_project / residual_term_fold_spatial), every other reader folds it in (residual_materialize).
// residual_run / ssub_residual move NONE -> VIRTUAL | RESIDENT, residual_realize VIRTUAL -> RESIDENT, residual_materialize pending -> applied.
struct ResidualState {
    rplan::Form form = rplan::NONE;
    int source = rplan::SRC_NONE;      // who wrote it: 1 = cnmfe_residual, 2 = cnmfe_residual_ssub (compute_RSS / reconstruct_background serve 1 only)
    int64_t gen = 0;                   // counts the requests of this patch: what a projection queued ahead of its consumer is valid for
    bool has_pending = false;
    bool solve_marked = false;         // option ring_side: W of this patch is final behind cnmfe_ctx::ev_ring_solved (the event a ring fit records right behind its
                                       // solve) and nothing has invalidated since -- whatever changes W, b0 or the video goes through invalidate()
    FootTerm applied, pending;
    bool valid() const { return form != rplan::NONE; }
    bool is_virtual() const { return form == rplan::VIRTUAL; }
    void invalidate() { form = rplan::NONE; source = rplan::SRC_NONE; has_pending = false; solve_marked = false; applied.ac = false; }      // frees nothing; gen keeps counting
    rplan::TermsView terms() const { return {has_pending, applied.view(), pending.view()}; }
};

// what the last low-rank background fit of a patch did (bg_svd.hpp; cnmfe_bg_svd_stats): video passes, iterations, the relative residual
// |M u_i - theta_i u_i| / theta_1 and the singular value of every component, and whether every residual met the tolerance before the iteration cap
struct SvdStats { int64_t passes = 0, iters = 0; int converged = 0; int nb = 0; double resid[8] = {}, sv[8] = {}; };

// ---- per-patch resident state ----------------------------------------------------
struct Patch {
    int32_t prect[4], brect[4];        // 1-based inclusive [r0 r1 c0 c1]
    int32_t d1 = 0, d2 = 0;
    int32_t nr = 0, nc = 0, nr_b = 0, nc_b = 0;
    int32_t roff = 0, coff = 0;        // patch origin inside the block (0-based)
    int64_t T = 0, d = 0, d_b = 0;
    DevBuf Y;                          // upload staging: T x d_b fp32, frame-major; released once Yc4 is built
    DevBuf Yc4;                        // the RESIDENT video: centred (Y - Ymean), 4-frame interleaved: [ceil(T/4)][d_b] float4
    int64_t Tc = 0;                    // ceil(T/4)
    DevBuf ymean_d;                    // d_b double
    DevBuf ymean_f;                    // d_b float
    bool ymean_valid = false;
    int64_t frames_uploaded = 0;       // distinct frames that have arrived
    std::vector<uint8_t> frame_seen;   // T flags: a frame counts once, overlapping or repeated chunks are rejected (cnmfe_upload_block)
    // ring
    int32_t radius = 0, p = 0;         // p ring offsets
    std::vector<int32_t> dr, dc;       // ring offsets, (dc, dr)-sorted == MATLAB find() order
    DevBuf ring_dr, ring_dc;           // int32[p]
    DevBuf W;                          // p x d fp32, offset-major; 0 where the neighbour is outside the FOV
    DevBuf b0;                         // d fp64 (kept in double on the device; the ABI converts)
    bool ring_ready = false;
    DevBuf sn_b;                       // d_b fp32 noise levels of the block pixels (cnmfe_set_noise): only the outlier branch of the ring fit reads them
    bool sn_ready = false;
    // background_model = 'svd' (bg_svd.hpp): b (nb columns of d), f (nb rows of T), b0 (d), all fp64; svd_nb = -1: none yet (cnmfe_bg_svd_fit / cnmfe_bg_svd_set)
    DevBuf svd_b, svd_f, svd_b0; int svd_nb = -1; SvdStats svd_stats;
    DevBuf ysig;                       // Ysig4[ceil(T/4)][d] float4, the background-subtracted video of this patch where it is resident; `residual` says what it holds
    ResidualState residual;
    // P(j,k) = sum_t Yc_j(t) Cc_k(t) in fp64 per 16x16 block of the block region and list slot: pt_tab[(pt_lp[b] + slot) * 256 + lp_of(pixel)], pt_slot[b * pt_K + k]
    // = slot or -1.  The ring fit's window projection computes exactly this (all frames, the same centred traces) and leaves it here; otherwise the
    // spatial update builds it.  Columns are rows pt_rows[] of the bound trace matrix of generation pt_gen (-1: some other matrix -- not reusable).
    DevBuf pt_tab, pt_lp, pt_slot;
    bool pt_valid = false; int32_t pt_K = 0; int64_t pt_gen = -1;
    std::vector<int32_t> pt_rows; std::vector<int> pt_lp_h; std::vector<short> pt_slot_h;
    // incremental ring regression (bg.hip): the block-pair covariance table and row sums of the centred VIDEO (no footprints subtracted),
    // valid for one frame stride until the video changes
    DevBuf cov_base, rowsum_base;
    bool base_valid = false, derived = false;             // derived: a low-resolution patch of bg_ssub > 1 (its video is rebuilt every call)
    int base_kstride = 0;
    // a second table of the same video at ANOTHER frame stride: the stride follows pmax (fit_ring_model.m:84-87: k = floor(T / min(T, 100 pmax))), and a
    // recording whose T / (100 pmax) sits at an integer -- T = 20000 with pmax around 66 -- alternates between two strides from fit to fit; one kept table
    // meant a full fp64 rebuild (10-15 ms per patch) on every flip.  Allocated only when a second stride turns up.
    DevBuf cov_base_alt, rowsum_base_alt; bool base_alt_valid = false; int base_alt_kstride = 0;
    // The block-pair tables of the ring fit (ring_plan.hpp: ring_pairs, ring_tables) on the host and the device.  They follow the block geometry and the ring offsets
    // only -- not A, C or the frame stride -- so they stay with the patch under the key they were computed from (bg.hip, fit_pair_tables / fit_need_tables): a fit
    // whose kernels read none of them (the steady-state packed fit) neither computes nor uploads them, and a table swap between two frame strides leaves them alone.
    struct RingTabs {
        bool keyed = false, built = false;                 // key / npairs hold; the host vectors and the device copies hold
        int geo[8] = {0, 0, 0, 0, 0, 0, 0, 0}; std::vector<int32_t> dr, dc;      // the key: nr_b, nc_b, roff, coff, nr, nc, p_radius, maxd + the ring offsets
        int npairs = 0, nwork = 0;
        std::vector<plan::Pair> pairs; std::vector<int> pair_of; plan::Tables tabs;
        DevBuf dPairs, dPairOf, dWork, dNeed, dTcnt, dTl;
    } rt;
    // the video's normal equations per patch pixel, packed in the ring solve's register-tile order (ring_solve_packed.hpp): gathered once from cov_base
    // (and once more for a second frame stride), 43 KB per pixel at p = 96
    DevBuf sys, sys_alt; bool sys_valid = false, sys_alt_valid = false;
    // round 6 (ring_solve_inv.hpp): the explicit inverses of those systems at a ridge lam0 per pixel (k_ring_inverse: built behind the patch's first packed fit,
    // the bytes of `sys` once more), the ridge every fit leaves per pixel, and the list of pixels a fit's fast path (k_ring_apply) left to k_ring_solve6
    // (kinv_list: [d] pixels, then 4 counters).  They belong to `sys`: invalid whenever it is
    DevBuf kinv, kinv_lam, kinv_list; bool kinv_valid = false, kinv_lam_valid = false; int kinv_fits = 0;
    void drop_inverses() { kinv_valid = false; kinv_lam_valid = false; kinv_fits = 0; }
    void drop_systems() { sys_valid = false; drop_inverses(); }
    // the centred video as 32-bit fixed-point digit planes [blk][frame/16][plane][256 px] x 16 B + per-pixel scales (gram_i8.hpp), kept for the fits' window projection
    // (win_proj_i8.hpp) when the memory allows: frame stride 1 only
    DevBuf dig, dig_sc; int64_t dig_T16 = 0; bool dig_valid = false;
    DevBuf yt4; bool yt4_valid = false;                   // vproj.hip: the centred video tiled by 16 x 16 block (k_tile_video), for the temporal projection
    DevBuf digp; bool digp_valid = false;                 // vproj_i8.hpp: the digit planes once more, pixel-major (k_dig_pixmajor), for the temporal projection on the int8 pipe
    // bg_ssub > 1 (ssub.hip, round 5: the sweep-free residual of source 2): the low-resolution residual patch and the factor of the last cnmfe_residual_ssub, and
    // imresize's bicubic UPSAMPLING taps of the block region's rows / columns (low-resolution index + weight, ss_Pr / ss_Pc per row / column) on the host and the
    // device, their ranges per row / column (made monotone: ss_rlo[r] <= every tap index of the rows >= r, ss_rhi[r] >= those of the rows <= r), and the
    // TRANSPOSED taps (per low-resolution row / column the block-region rows / columns it feeds, CSR) for up' A of the temporal projection
    int ss_res = -1, ss_ssub = 0, ss_Pr = 0, ss_Pc = 0, ss_d1s = 0, ss_d2s = 0;
    bool ss_taps = false;
    std::vector<int> ss_tr_idx, ss_tc_idx, ss_rlo, ss_rhi, ss_clo, ss_chi, ss_trp_h, ss_tri_h, ss_tcp_h, ss_tci_h;
    std::vector<float> ss_tr_w, ss_tc_w;
    DevBuf ss_ir, ss_wr, ss_ic, ss_wc, ss_trp, ss_tri, ss_trw, ss_tcp, ss_tci, ss_tcw, ss_dlt;
    // what the next fit asks of W before it can queue anything (pmax of fit_ring_model.m:60, row 1 for the first-run test of :25), copied to
    // pinned memory behind the fit that produced W: the next fit reads it without draining the stream (ring_stats_*, api.hip)
    DevBuf stat_dev; void *stat_host = nullptr; hipEvent_t stat_ev = nullptr; bool stat_valid = false;
    int lane = 0;                                          // the execution lane (stream + scratch set) of this patch's calls: cnmfe_ctx::activate, option "lanes"
    PeelSession *peel = nullptr;                           // an open greedy-initialisation session (cnmfe_peel_open)
    ~Patch() { delete peel; if (stat_host) (void)hipHostFree(stat_host); if (stat_ev) (void)hipEventDestroy(stat_ev); }
};

// device scratch of the OASIS kernels (deconv.hip): pool / task tables, grown on demand and kept with the context
struct DeconvScratch { DevBuf pv, pw, pt, pl, tkp, tko, tkl, tkv, pnum, list, ybuf, obuf, tbuf; };      // (moves member by member: DevBuf)

// One patch's temporal update set up but not swept (cnmfe_hals_temporal_job): its projections, A'A lists and traces in buffers of its own, its
// Gauss-Seidel level schedule on the host.  cnmfe_temporal_jobs_sweep then runs level l of EVERY job of the context in one launch -- the patches of a
// rank are independent (update_temporal_parallel.m:112-186 is a parfor over them), and a level is a handful of workgroups whose duration is one
// trace's chain of work: sixteen patches' levels one after the other leave the chip empty sixteen times as long.
struct TemporalJob {
    Patch *P = nullptr; int32_t K = 0; int64_t ldc = 0, T = 0; int maxIter = 0; bool deconv = false; cnmfe_deconv_opts dopts{};
    DevBuf dC, dColptr, dErow, dAval, dU, dCraw, dNk, dNidx, dNval, dNptr, dAa, dOvf, dS, dPars, dSn, dB;
    std::vector<std::vector<int>> levels;
    bool swept = false;
    bool dag = false;                                      // `levels` are the levels of the dependency graph over the items of all maxIter sweeps (factor.hip, dag_schedule)
    // A'A of the job comes back into pinned memory WITHOUT a wait in cnmfe_hals_temporal_job (the host goes on to the next patch); the sweep call waits once
    // for all jobs and finishes each: aa = diag(A'A) against the host-side column test, the projection again if a footprint term overflowed its list
    std::vector<int> diag; std::vector<char> upd; bool term_applied = false, finished = false; int nn = 0;
    float *pin = nullptr; size_t pin_cap = 0;             // nn floats of A'A values + one int (the term-projection overflow word)
    // initTemporal (init_temporal.hpp): the stitch weights are NOT the regression's aa (dAa, the squared norms of the ring-filtered footprints) but AA of the
    // original footprints on the patch rows (initTemporal.m:160,285): cnmfe_stitch_add_job takes dW when has_w
    DevBuf dW; bool has_w = false;
    // ... and its deconvolution sweeps run on the CENTRED video's U: dOff (K doubles) is what the raw video adds to each row, which GetSn alone sees (deconv.hip, DeconvIO::off)
    DevBuf dOff; bool has_off = false;
    ~TemporalJob() { if (pin) (void)hipHostFree(pin); }
};

}  // namespace cnmfe

namespace cnmfe {
// Pinned staging for the small host -> device uploads of a call (index lists, CSR arrays, tables).  to_dev() copies the caller's data into
// the arena and enqueues the transfer from there, so (a) the source may go away as soon as to_dev returns and (b) the call does not have to
// drain the stream for that -- the host prepares the next patch while the GPU still works on this one.  Two halves: before allocating in a
// half again, the host waits for the event that marks the last transfer enqueued out of it.
struct PinArenaFields { char *p = nullptr; size_t cap = 0, off = 0; int half = 0; hipEvent_t ev[2] = {nullptr, nullptr}; bool ev_set[2] = {false, false}; };
struct PinArena : PinArenaFields {
    PinArena() = default;
    PinArena(const PinArena &) = delete; PinArena &operator=(const PinArena &) = delete;
    // a move steals the arena and its events and leaves the source empty (the fields as a whole: no list of them here)
    PinArena(PinArena &&o) noexcept : PinArenaFields(o) { static_cast<PinArenaFields &>(o) = PinArenaFields(); }
    PinArena &operator=(PinArena &&o) noexcept {
        if (this != &o) { release(); static_cast<PinArenaFields &>(*this) = o; static_cast<PinArenaFields &>(o) = PinArenaFields(); }
        return *this;
    }
    void release() { if (p) (void)hipHostFree(p); for (int i = 0; i < 2; ++i) if (ev[i]) (void)hipEventDestroy(ev[i]); static_cast<PinArenaFields &>(*this) = PinArenaFields(); }
    int init(size_t bytes) {
        if (p) return 0;
        if (hipHostMalloc((void **)&p, bytes, hipHostMallocDefault) != hipSuccess) { p = nullptr; return -1; }
        cap = bytes;
        for (int i = 0; i < 2; ++i) if (hipEventCreateWithFlags(&ev[i], hipEventDisableTiming) != hipSuccess) return -1;
        return 0;
    }
    // nullptr: the request does not fit half the arena (the caller copies straight from its buffer and waits)
    template <class F> void *take(size_t n, F &&stream_of) {      // stream_of(): asked for only when the halves switch (it sends the held-back uploads first)
        n = (n + 255) & ~size_t(255);
        if (!p || n > cap / 2) return nullptr;
        const size_t end = (size_t)(half + 1) * (cap / 2);
        if (off + n > end) {
            (void)hipEventRecord(ev[half], stream_of()); ev_set[half] = true;
            half ^= 1; off = (size_t)half * (cap / 2);
            if (ev_set[half]) (void)hipEventSynchronize(ev[half]);
        }
        void *r = p + off; off += n; return r;
    }
    ~PinArena() { release(); }
};
}  // namespace cnmfe

namespace cnmfe {
// Small uploads out of the pinned arena are not enqueued one by one: to_dev() notes (destination, arena slot, length) here, and whatever next asks for
// the stream -- a launch, a memset, a copy, a wait: cnmfe_ctx::st() -- first sends all of them as ONE copy kernel.  A call's ten or twenty index
// lists and tables then cost one dispatch instead of one each (44 per patch and iteration in the 4 x 4-patch configuration: 700 dependent
// 4-microsecond dispatches, 6 ms of GPU time line per iteration, profiles/r03/gap_analysis_c4.txt).
constexpr int PIN_NSEG = 24;
// int8 matrix pipe, sums over FRAMES (gram_i8.hpp, win_proj_i8.hpp): 4 digit pairs x 64 frames x 2^14 per accumulation step keep an int32 sum exact for this many frames
constexpr int I8_SEG_FRAMES = 24576;
struct PinSegs { const uint4 *src[PIN_NSEG]; uint4 *dst[PIN_NSEG]; unsigned n16[PIN_NSEG]; };
}  // namespace cnmfe

// Execution lanes (option "lanes", round 6).  The patches of a rank are independent inside each of the three updates (the reference's parfor), and most of a small
// patch's kernels are a few workgroups with 8-10 us of dispatch latency between two dependent ones: on ONE stream sixteen 128 x 128 patches leave the chip idle for a
// sixth of the iteration.  A lane is a stream + a full set of the context's per-call scratch (+ its own pinned upload arena and held-back uploads): LaneState, THE list
// of what a lane owns.  The context derives from it -- its own LaneState is the active lane's -- and a stored lane (cnmfe_lane) holds one; a patch belongs to lane
// (creation order) mod lanes, every call with a patch id ACTIVATES the patch's lane first (get_patch), and the two states change places as a whole (cnmfe_lane::store / load: moves), so that no
// code path knows about lanes and a member added here is a member of every lane.  Calls without a patch id that touch what all patches share (the bound traces, the
// stitch accumulator, the temporal jobs' sweep, post-processing) run on lane 0 after lane 0 has been made to wait for the other lanes (join), and leave an event the
// other lanes wait for at their next activation (fork) -- cnmfe::GlobalScope.  lanes = 1 (the default): none of this does anything.  ("Lane state and kept results")
namespace cnmfe {
struct LaneState {
    hipStream_t stream_ = nullptr;                         // the compute stream (owned by whoever holds the state: ~cnmfe_ctx the active one, ~cnmfe_lane a stored one)
    PinSegs pseg{}; int npseg = 0;                         // the held-back small uploads (cnmfe_ctx::st)
    PinArena pin;
    DevBuf vp[32];            // scratch of the sweep-free projections (vproj.hip; [16..]: the bg_ssub > 1 forms)
    int64_t last_ldc = 0;     // row stride of the centred traces the last residual_run left in tmp[1]
    DevBuf ysig_low;          // bg_ssub > 1: residual sweep of the low-resolution patch
    DevBuf up_tmp;            // bg_ssub > 1: column-upsampled W*(...) (low rows x block columns)
    DevBuf bgs_r, bgs_b, bgs_upr, bgs_upc;   // bg_ssub > 1, reconstruct_background / compute_RSS: R_low, W*R_low, replication maps
    int bgs_patch = -1, bgs_d1s = 0; int64_t bgs_dF = 0;   // the patch bgs_b belongs to (cnmfe_background_ssub)
    DevBuf bf;                // tiled centred background residual  [blk][t'][256] fp32
    DevBuf dig_smax;          // gram_i8.hpp: per block-region pixel max |Bf| (float bits) of the build in flight
    DevBuf dig_rspart;        // gram_i8.hpp: per frame chunk the row sums of the build in flight (reduced in a fixed order by k_rs_reduce)
    DevBuf dig_scale;         // gram_i8.hpp: per block-region pixel the scale of its 32-bit fixed-point trace (the int8-digit table build)
    DevBuf tdig, tscale, gk, win_items;   // win_proj_i8.hpp: digit planes / scales of the centred traces, their K x K Gram matrix, the (block, trace group) work items
    DevBuf bf2, outl_cnt, outl_sel;   // outlier branch of the ring fit: clipped copy of bf, outliers per frame, kept frames
    DevBuf cov;               // block-pair covariances [pair][256][256] (fp64)
    DevBuf rowsum;            // [blk][256] double
    DevBuf tmp[16];           // small scratch
    DevBuf inc[7];            // incremental ring regression: block footprint lists, U~, trace sums
    DevBuf stg[4];            // ring_solve_staged.hpp: per-neuron window metadata, per-list-position metadata, the windows of U~ and of A
    DevBuf wcodes, solve_fill;   // ring solve: the block-pair codes per window origin (k_win_codes); the fill values {0, 1} in global memory (ring_solve.hpp)
    DevBuf stage;             // upload staging
    DevBuf dfl[5];            // dff.hpp: [0] the frame chunk of the reconstructed background (<= 256 MB), [1..4] the call's A (colptr, rowidx, val) and accumulator rows
    DevBuf dmx[6];            // demix.hpp: [0..2] the call's A as CSR over the patch pixels, [3] its trace rows, [4] its colours, [5] the six panels on their way to the host
    // per-call device scratch of the factor updates (factor.hip, deconv.hip): grown on demand, NEVER freed between calls -- a hipMalloc /
    // hipFree pair per buffer and call cost more than the small kernels they serve, and hipFree drains the device
    DevBuf scr[24];
    DevBuf svd[19];           // bg_svd.hpp: the panels Q, Z, G, D, the passes' partial sums, the small products, the call's A as CSC and CSR
    DevBuf itl[16];           // init_temporal_lowrank.hpp: M = [A_p, b] as CSC (fp64), the pair list, G, the Cholesky tiles, R | Y | X of the solve
    DevBuf itp[30];           // init_temporal.hpp: the block's footprints, the ring-filtered footprints and their rough-start selection (fp64), their lists, U | C0 of the projection
    DeconvScratch dscr;
    kept::KeptSpatial kept;   // what the last deferred spatial update of this lane left in scr[SCR_COLPTR | SCR_EROW | SCR_AVAL | SCR_KEEP] (kept_results.hpp)
    LaneState() = default;
    LaneState(LaneState &&) = default; LaneState &operator=(LaneState &&) = default;
};
}  // namespace cnmfe

struct cnmfe_lane {
    cnmfe::LaneState state;                                                  // this lane's members while another lane is the active one (empty while it is active)
    // a lane switch is two moves of a whole state (two std::swaps cost three moves each: 1.0 us per switch on the host against 0.32)
    void store(cnmfe::LaneState &active) { state = std::move(active); }
    void load(cnmfe::LaneState &active) { active = std::move(state); state.stream_ = nullptr; }   // (the stream is a raw handle: the move copied it, and ~cnmfe_lane destroys what it finds here)
    hipEvent_t ev = nullptr; int64_t fork_seen = 0; bool dirty = false;      // (these three describe the lane itself and never change places)
    ~cnmfe_lane() { if (state.stream_) (void)hipStreamDestroy(state.stream_); if (ev) (void)hipEventDestroy(ev); }
};

struct cnmfe_ctx : cnmfe::LaneState {
    int device = 0;
    void flush_copies();                                   // api.hip
    hipStream_t st() { if (npseg) flush_copies(); return stream_; }   // the compute stream, every held-back upload enqueued first (npseg: written by this context's own thread only, pin_flush_range)
    hipStream_t copy_stream = nullptr;                     // device -> pinned host downloads that should not hold up the compute stream
    // option fit_side (bg.hip, SideScope): the second stream a steady-state ring fit queues its set-up on, beside the window projection; created at its first use at
    // the compute stream's priority, with the event the side stream waits for (fork) and the one the compute stream waits for (join)
    hipStream_t side_stream = nullptr; hipEvent_t ev_side_fork = nullptr, ev_side_join = nullptr;
    // option ring_side (SideScope::fork_behind below; resid.hip, ring_side_ahead): ev_ring_solved is recorded right behind a ring fit's solve, and the fit
    // queues the statistics of the new W and the W*A tables of the residual request that follows it on the side stream behind THAT event, beside whatever the compute
    // stream is given next; ev_ring_join marks their end, and ring_side_join() makes the compute stream wait for it (ring_join_pending: not yet) -- in the next
    // residual request, the next fit, the calls that write W, cnmfe_synchronize.  rsd: [0] the CSR rows of A, [1..3] the tables (they change hands with the
    // patch's pending term as tmp[8..10] do); rs_pin: the pinned staging of [0], the scope's own (the shared arena's half-switch events assume one stream at a time)
    hipEvent_t ev_ring_solved = nullptr, ev_ring_join = nullptr; bool ring_join_pending = false, ring_join_used = false;
    cnmfe::DevBuf rsd[4]; void *rs_pin = nullptr; size_t rs_pin_cap = 0;
    // the tables in rsd[1..3]: of which patch and which A (the fit's CSC arrays, compared with the request's before anything of the request is built)
    struct RingAhead {
        bool valid = false; const cnmfe::Patch *P = nullptr; int32_t K = 0; std::vector<int64_t> colptr; std::vector<int32_t> rowidx; std::vector<float> val;
        void keep(const cnmfe::Patch *P_, int32_t K_, const int64_t *cp, const int32_t *ri, const float *va) {
            P = P_; K = K_; colptr.assign(cp, cp + K_ + 1); rowidx.assign(ri, ri + cp[K_]); val.assign(va, va + cp[K_]); valid = true;
        }
        bool is(const cnmfe::Patch *P_, int32_t K_, const int64_t *cp, const int32_t *ri, const float *va) const {
            return valid && P == P_ && K == K_ && memcmp(colptr.data(), cp, (size_t)(K_ + 1) * sizeof(int64_t)) == 0
                   && memcmp(rowidx.data(), ri, rowidx.size() * sizeof(int32_t)) == 0 && memcmp(val.data(), va, val.size() * sizeof(float)) == 0;
        }
    } rs_ahead;
    int ring_side_join() {
        if (!ring_join_pending) return 0;
        ring_join_pending = false;
        return hipStreamWaitEvent(st(), ev_ring_join, 0) == hipSuccess ? 0 : cnmfe::fail(CNMFE_EHIP, "ring_side: the compute stream could not wait for the side stream");
    }
    hipEvent_t ev_bound_ready = nullptr, ev_copy_done = nullptr; bool copy_pending = false;
    // every batch of downloads on the copy stream gets a generation number and an event of its own: a host buffer waits for ITS batch (cnmfe_copy_wait),
    // not for whatever was queued on the copy stream since (cnmfe_stitch_wait) -- releasing last iteration's traces must not wait for this iteration's
    int64_t copy_gen = 0; std::vector<std::pair<int64_t, hipEvent_t>> copy_gens; std::vector<hipEvent_t> copy_ev_pool;
    int copy_batch_mark();                                 // api.hip: after the last enqueue of a batch on copy_stream
    std::vector<hipEvent_t> tickets; std::vector<char> ticket_busy;   // cnmfe_update_spatial_fetch_async / cnmfe_ticket_wait
    int *ticket_flags = nullptr;                           // pinned, TICKET_FLAGS words: what the kernels in front of ticket t raised since the previous take (k_flag_take: read and cleared at the ticket's place in the stream)
    cnmfe::DevBuf ticket_dev;                              // the device side of those words
    static constexpr size_t TICKET_FLAGS = 1024;
    cnmfe::Profiler prof;
    std::map<int, cnmfe::Patch *> patches;
    // shared by all patches and all lanes of this context
    cnmfe::DevBuf bound;      // trace matrix bound with cnmfe_traces_bind (K x ldc fp32), passed as c_order = CNMFE_BOUND
    int32_t bound_K = 0; int64_t bound_T = 0; int bound_order = 1; bool bound_valid = false;
    int64_t bound_gen = 0;    // counts the changes of the bound matrix' CONTENT (cnmfe_traces_bind, the stitch, deconvTemporal on it): what a table derived from its rows is valid for
    // high-water sizes of the buffers that change hands between the scratch and the patches (DevBuf::ensure_hw): vp[], and what rotates through tmp[1], tmp[2],
    // tmp[8..10].  They stay with the context: what one lane's patches needed, the other lanes' buffers get at once
    size_t hw_vp[32] = {}, hw_cc = 0, hw_cm = 0, hw_wa[3] = {0, 0, 0};
    // the traces the last cnmfe_hals_temporal[_deconv] / cnmfe_fast_temporal left on the device (C_raw rows of stride ldc, and aa): what cnmfe_stitch_add folds
    // into the stitch accumulator without a host round trip.  Written by the non-job temporal updates only, void while one runs, consumed by the stitch
    struct LastTemporal { cnmfe::DevBuf craw, aa; int32_t K = 0; int64_t ldc = 0, T = 0; bool valid = false;
        void set(int32_t K_, int64_t ldc_, int64_t T_) { K = K_; ldc = ldc_; T = T_; valid = true; } } last_t;
    // The temporal projection queued behind the connectivity kernel (option temporal_early, factor.hip: temporal_early_project; DESIGN.md section 3, "the hand-over").
    // a: keep ? value : 0 on the mask's pattern; u: U = B' Yc of exactly those values.  Nothing else writes either.  The tag (kept_results.hpp) says what u is valid
    // for; temporal_run takes it only when the caller claimed the token (its A IS that spatial result) and every field still holds, and drops it otherwise.
    struct EarlyU : cnmfe::kept::EarlyTag { cnmfe::DevBuf a, u; int64_t nent = 0; } early;      // nent: (block, neuron) entries of that projection (a counter)
    int64_t spatial_gen = 0;                                             // spatial results so far, over all lanes (KeptSpatial::gen, EarlyTag::spatial_gen)
    int64_t last_nent = 0;                                               // (block, neuron) entries of the last vproj_temporal
    int64_t early_seq = 0, early_hits = 0, early_drops = 0, early_declined = 0, sweep_nowait = 0;   // counters (cnmfe_get_option)
    std::vector<cnmfe::TemporalJob *> tjobs; int tjobs_used = 0;          // cnmfe_hals_temporal_job: kept (with their buffers) from update to update, counted from cnmfe_stitch_begin
    cnmfe::DevBuf dcv_c, dcv_s, dcv_pars, dcv_sn;          // cnmfe_deconv_temporal_bound: C_raw - b (after the swap with `bound`), S, kernel_pars, sn -- read by the copy stream, so not shared scratch
    // merging (merge.hpp): dcv_c / dcv_s / dcv_pars / dcv_sn are the C_raw, S, kernel_pars, sn that belong to the bound matrix C while residents_gen == bound_gen
    // (cnmfe_deconv_temporal_bound, cnmfe_traces_load, cnmfe_merge_apply set it; every other change of the bound matrix' content leaves it behind)
    int64_t residents_gen = -1; bool res_has_s = false;
    cnmfe::DevBuf mrg[23];                                 // [0] an uploaded source, [1] the result of cnmfe_trace_diff_spikes (diff_K x diff_T), [2..5] moments / K x K / sn, [6..22] cnmfe_merge_apply
    int32_t diff_K = 0; int64_t diff_T = 0;
    cnmfe::DevBuf fpo[4];                                  // footprint image operations (footprint_ops.hpp): [0] the boxes' offsets, [1] the result, [2] the structuring element, [3] counts
    int64_t image_ops_host = 0;                            // counter image_ops_host_columns: columns the last such call left to the caller (box above FP_MAX_CELLS)
    int64_t trace_uploads = 0;                             // counter trace_matrix_uploads: K x T matrices ANY entry point took through a pointer (upload_traces; a bound matrix or rows of it do not count)
    int64_t itl_reads = 0, itl_factor_us = 0;             // counters init_temporal_lowrank_video_reads / _factor_us: projection passes and the host factorisation's time of the last cnmfe_init_temporal_lowrank
    int64_t last_nlevels = 0;                              // counter init_temporal_levels: launches of level kernels the last cnmfe_init_temporal queued itself (the depth of its schedule)
    int64_t merge_uploads = 0;                             // counter merge_trace_uploads: K x T matrices the merge / tag entry points took from the host
    // dF/F (dff.hpp): the K x T fp64 accumulator of cnmfe_df_begin .. cnmfe_df_finish (row stride df_T), and [0] 1 / sum(A.^2), [1] the rows that are not finite, [2] Df,
    // [3] a divided matrix on its way out.  ev_df chains the projections of different lanes in call order (df_chain: one has been queued since cnmfe_df_begin)
    cnmfe::DevBuf df_acc, df_buf[4];
    int32_t df_K = 0; int64_t df_T = 0; bool df_open = false, df_chain = false;
    hipEvent_t ev_df = nullptr;
    // overlap-region stitch of update_temporal_parallel.m:264-280: acc[k][0..T) = sum_m aa_m(k) C_raw_m(k,:), acc[k][ld-1..] ... see cnmfe_stitch_begin
    cnmfe::DevBuf stitch;     // K rows of stitch_ld floats: [0, T) the weighted sum, column stitch_ld - 4 the sum of the weights
    int32_t stitch_K = 0; int64_t stitch_T = 0, stitch_ld = 0; bool stitch_open = false;
    void *rccl_comm = nullptr; int rccl_rank = 0, rccl_n = 0;          // single-process multi-GPU stitch (cnmfe_stitch_temporal)
    cnmfe::DevBuf errflag;    // one int, set by kernels that meet a state the host-side set-up should have excluded (checked at the next sync)
    std::map<std::string, int64_t> opts;
    int trace_level = 0;                                   // opts["host_trace"], read by every LAUNCH
    int64_t opt(const char *n, int64_t dflt) const { auto it = opts.find(n); return it == opts.end() ? dflt : it->second; }
    // lanes (see LaneState): lanes[k] holds lane k's state while another lane is active; empty = one lane
    std::vector<cnmfe_lane *> lanes; int cur_lane = 0, patches_created = 0;
    int spatial_lane = 0;                                  // the lane of the last cnmfe_update_spatial (the fetch calls carry no patch id)
    hipEvent_t ev_fork = nullptr; int64_t fork_gen = 0;
    int activate(int lane);                                // api.hip: make `lane` the active one (its stream behind st(), its scratch behind the members)
    int join_lanes();                                      // api.hip: lane 0 active and waiting for everything the other lanes have been given
    int fork_mark();                                       // api.hip: the other lanes wait for what lane 0 has been given up to here, at their next activation
    void patches_changed();                                // api.hip: a patch was created or replaced -- no lane's record and no queued projection names a patch any more
    ~cnmfe_ctx();
};

namespace cnmfe {
// the options that select the kernel of the temporal projection, with their defaults: the one place that names them
inline kept::ProjOpts proj_opts(const cnmfe_ctx *ctx) { return {ctx->opt("proj_i8", 1), ctx->opt("proj_i8_planes", 3), ctx->opt("proj_tiled", 1)}; }
// the guard of the three fetch calls: the active lane still holds the deferred result of nnz values (connected: and its pattern)
inline int require_kept_spatial(const cnmfe_ctx *ctx, int64_t nnz, bool connected) {
    if (connected ? ctx->kept.fetchable_connected(nnz) : ctx->kept.fetchable(nnz)) return 0;
    return fail(CNMFE_ESTATE, "no deferred spatial update of %lld values (last one: %lld)", (long long)nnz, (long long)ctx->kept.nnz);
}
}  // namespace cnmfe

namespace cnmfe {
// option "host_trace" = 1: wall-clock marks of the host-side phases of a call on stderr (scripts/host_timeline.py)
struct HostTrace {
    bool on; const char *name; std::chrono::steady_clock::time_point t0, last;
    HostTrace(cnmfe_ctx *ctx, const char *n) : on(ctx->opt("host_trace", 0) != 0), name(n) { if (on) t0 = last = std::chrono::steady_clock::now(); }
    void mark(const char *what) {
        if (!on) return;
        const auto t = std::chrono::steady_clock::now();
        fprintf(stderr, "[host_trace] %s: %-28s %8.3f ms (at %8.3f)\n", name, what, std::chrono::duration<double, std::milli>(t - last).count(),
                std::chrono::duration<double, std::milli>(t - t0).count());
        last = t;
    }
};
// (a call with a patch id runs on the patch's lane: its stream and its scratch are the context's from here on)
inline Patch *get_patch(cnmfe_ctx *ctx, int id) {
    auto it = ctx->patches.find(id);
    if (it == ctx->patches.end()) return nullptr;
    if (!ctx->lanes.empty() && ctx->activate(it->second->lane) != 0) return nullptr;
    return it->second;
}
// a call WITHOUT a patch id that reads or writes what the patches share: lane 0, behind everything the other lanes were given; what it queues is waited for by
// the other lanes' next calls
struct GlobalScope {
    cnmfe_ctx *ctx; int rc = 0;
    explicit GlobalScope(cnmfe_ctx *c) : ctx(c) { if (ctx && !ctx->lanes.empty()) rc = ctx->join_lanes(); }
    ~GlobalScope() { if (ctx && !ctx->lanes.empty()) (void)ctx->fork_mark(); }
};
int pinned_to_dev(cnmfe_ctx *ctx, void *dst, const void *src_pinned, size_t bytes);   // api.hip
void pin_register(cnmfe_ctx *ctx, bool live);
// upload a host vector to a DevBuf on the context stream
template <class T> inline int to_dev(cnmfe_ctx *ctx, DevBuf &b, const T *h, size_t n) {
    RET(b.ensure(std::max<size_t>(n, 1) * sizeof(T)));
    if (!n) return 0;
    if (void *st = ctx->pin.take(n * sizeof(T), [ctx] { return ctx->st(); })) {             // staged: `h` is free again when this returns
        memcpy(st, h, n * sizeof(T));
        // small uploads go by a copy KERNEL that reads the pinned arena over PCIe, not by hipMemcpyAsync: the copy engine also serves the big asynchronous
        // downloads of the traces (20-60 MB behind every temporal update), and an upload of a few KB queued behind one of those held the next call's first
        // kernel back by 0.5-1.5 ms (profiles/r03/gap_analysis_*.txt)
        return pinned_to_dev(ctx, b.p, st, n * sizeof(T));
    }
    CK(hipMemcpyAsync(b.p, h, n * sizeof(T), hipMemcpyHostToDevice, ctx->st()));
    CK(hipStreamSynchronize(ctx->st()));                                   // too large for the arena: straight from the caller's buffer
    return 0;
}
template <class T> inline int to_dev(cnmfe_ctx *ctx, DevBuf &b, const std::vector<T> &h) { return to_dev(ctx, b, h.data(), h.size()); }
// [k][t] row-major fp32 copy of a K x T matrix given in `order`; device result has row stride ldc (multiple of 4)
int upload_traces(cnmfe_ctx *ctx, DevBuf &dst, const float *C, int32_t K, int64_t T, int order, int64_t *ldc);
int download_traces(cnmfe_ctx *ctx, const float *dC, int64_t ldc, float *C, int32_t K, int64_t T, int order);

// implemented in the kernel translation units
int bg_fit_ring(cnmfe_ctx *ctx, Patch *P, int32_t K, const int64_t *A_colptr, const int32_t *A_rowidx, const float *A_val,
                const float *C, int c_order, int with_projection, float *b0_out, int64_t info[4], int b0_only = 0, double thresh_outlier = NAN);
int tu_warm_resid(); int tu_warm_bg();
int win_i8_table(cnmfe_ctx *ctx, Patch *P, const char *name_dig, const char *name_proj, int K, const float *dCc, int64_t ldc, const std::vector<int> &lst_ptr, const std::vector<int> &blall,
                 const int *dLp, const int *dLk, int nsg, double *dUt, int64_t ut_stride);   // bg.hip: the int8 window projection of all frames (the spatial update's table, vproj.hip)
int tu_warm_factor(); int tu_warm_deconv(); int tu_warm_ssub(); int tu_warm_vproj();   // one per translation unit: load its code object (cnmfe_create)
// bg.hip, THE memory rule: a buffer that has to grow to `bytes` may do so only if that leaves 8 GB of the device free (quarter: or a quarter of the device, if that is more)
int fits_leaving(const DevBuf &b, size_t bytes, bool *fits, bool quarter = false);
int bg_reserve(cnmfe_ctx *ctx, Patch *P);                 // bg.hip: the ring fit's large buffers, sized by the geometry, allocated ahead of the first fit
int residual_run(cnmfe_ctx *ctx, Patch *P, int pid, int32_t Ksel, const int64_t *A_colptr, const int32_t *A_rowidx,
                 const float *A_val, const float *C, int c_order, float *Ysig_out, int out_memspace, DevBuf *outbuf = nullptr, int tables_only = 0);
int ysig_export(cnmfe_ctx *ctx, Patch *P, DevBuf &ysig, float *Ysig_out, int out_memspace);
int rss_run(cnmfe_ctx *ctx, Patch *P, int32_t K, const int64_t *A_colptr, const int32_t *A_rowidx, const float *A_val, const float *C, int c_order,
            const float *b0_block, const float *b0_new, double *rss_out);
int bg_reconstruct_run(cnmfe_ctx *ctx, Patch *P, const float *b0_block, const float *b0_new, int64_t frame0, int64_t nframes, float *out, int out_memspace);
int residual_materialize(cnmfe_ctx *ctx, Patch *P);       // fold a pending footprint term into the resident Ysig (no-op without one); realizes a virtual residual first
rplan::ResidualOpts residual_opts(cnmfe_ctx *ctx);        // resid.hip: the residual's options with their defaults -- the one place that names them
int residual_realize(cnmfe_ctx *ctx, Patch *P);           // a VIRTUAL residual (ResidualState) becomes a resident one: the ring sweep runs now (no-op otherwise)
// rows of the bound trace matrix a (C, c_order) argument names: false when it is some other matrix
bool bound_rows_of(const cnmfe_ctx *ctx, const float *C, int c_order, int32_t K, std::vector<int32_t> &rows);
// vproj.hip -- the projections of a virtual residual.  Return 1 when they cannot serve the request (the caller realizes the residual and projects Ysig).
// (dQ != nullptr: instead of U, the ring sums sum_i W(m,i) P(m + o_i, k) of the mask's entries in fp64 -- what the bg_ssub form upsamples)
int vproj_spatial(cnmfe_ctx *ctx, Patch *P, int32_t K, const float *C, int c_order, const int64_t *IND_colptr, const int32_t *IND_rowidx,
                  const int *dErow, const int *dEcol, const float *dCc, int64_t ldc, float *dU, double *dQ = nullptr);
int vproj_temporal(cnmfe_ctx *ctx, Patch *P, int32_t K, const int64_t *A_colptr, const int32_t *A_rowidx, const float *A_val,
                   const int64_t *dColptr, const int *dErow, const float *dAval, float *dU, int64_t ldu, const double *dAval64 = nullptr, bool add_const = true);
// the same for a residual of cnmfe_residual_ssub (source 2): through the resampling maps, DESIGN.md section 3 bg_ssub
int vproj_spatial_ssub(cnmfe_ctx *ctx, Patch *M, int32_t K, const float *C, int c_order, const int64_t *IND_colptr, const int32_t *IND_rowidx,
                       const int *dErow, const int *dEcol, const float *dCc, int64_t ldc, float *dU);
int vproj_temporal_ssub(cnmfe_ctx *ctx, Patch *M, int32_t K, const int64_t *A_colptr, const int32_t *A_rowidx, const float *A_val,
                        const int64_t *dColptr, const int *dErow, const float *dAval, float *dU, int64_t ldu);
int ssub_taps(cnmfe_ctx *ctx, Patch *M, const Patch *R);  // ssub.hip: the upsampling taps of M's block region from R's grid, host + device (once per patch)
int ssub_realize(cnmfe_ctx *ctx, Patch *M);               // ssub.hip: the low-resolution sweep + upsample behind a virtual residual of source 2
int residual_term_project(cnmfe_ctx *ctx, Patch *P, int32_t K, const int64_t *dColptr, const int *dErow, const float *dAval, float *dU, int64_t ldu, int *dOverflow);   // 1: cannot be applied, materialise instead; *dOverflow set on the device if a footprint meets > 512 traces
int residual_term_fold_spatial(cnmfe_ctx *ctx, Patch *P, int32_t K, int64_t nnz, const int *dErow, const int *dEcol, const float *dCc, int64_t ldc, float *dU, DevBuf &dG);
int check_csc_pub(const char *what, int32_t ncol, int64_t nrow, const int64_t *colptr, const int32_t *rowidx);
int spatial_run(cnmfe_ctx *ctx, Patch *P, int algorithm, int32_t K, const int64_t *A_colptr, const int32_t *A_rowidx,
                const float *A_val, const float *C, int c_order, const int64_t *IND_colptr, const int32_t *IND_rowidx,
                const float *sn, int32_t param, float *A_out);
int temporal_run(cnmfe_ctx *ctx, Patch *P, int32_t K, const int64_t *A_colptr, const int32_t *A_rowidx, const float *A_val,
                 const float *C_in, int c_order, int32_t maxIter, float *C_out, float *C_raw_out, float *aa_out,
                 const cnmfe_deconv_opts *dopts, float *kernel_pars, float *S_out, float *sn_out, TemporalJob *job = nullptr);
// init_temporal.hpp (factor.hip): initTemporal.m:156-168 of one patch -- A: d_b x K CSC over BLOCK rows
int init_temporal_run(cnmfe_ctx *ctx, Patch *P, int32_t K, const int64_t *A_colptr, const int32_t *A_rowidx, const float *A_val, int32_t iters_plain, int32_t iters_last,
                      const cnmfe_deconv_opts *dopts, float *C_out, float *C_raw_out, float *S_out, float *pars_out, float *sn_out, float *AA_out, int c_order, TemporalJob *job = nullptr);
int vproj_pass_plan(Patch *P, int32_t K, const int64_t *colptr, const int32_t *rowidx, int per, std::vector<int> &pass_of, int reach = -1);   // vproj.hip
// init_temporal_lowrank.hpp (factor.hip): initTemporal.m:180-192 of one patch under background_model = 'svd' -- A: d_b x K CSC over BLOCK rows
int init_temporal_lowrank_run(cnmfe_ctx *ctx, Patch *P, int patch_id, int32_t K, const int64_t *A_colptr, const int32_t *A_rowidx, const float *A_val, int32_t iters_plain,
                              int32_t iters_last, const cnmfe_deconv_opts *dopts, float *C_out, float *C_raw_out, float *S_out, float *pars_out, float *sn_out, float *AA_out,
                              double *f_out, double *b0_out, int c_order);
// vproj.hip: R(row_of[j], :) = M(:, j)' Yc - cst[row_of[j]] in fp64 for ncol columns of a CSC matrix over PATCH rows with fp64 values; 1: a block meets more columns than its list holds
int vproj_columns64(cnmfe_ctx *ctx, Patch *P, int32_t ncol, const int64_t *colptr, const int32_t *rowidx, const int64_t *dColptr, const int *dErow, const double *dVal,
                    const int *dRowOf, const double *dCst, double *dR, int64_t ldr);
int temporal_sweep_jobs(cnmfe_ctx *ctx);                  // factor.hip: the level sweeps of every job set up since cnmfe_stitch_begin, level by level across the jobs
#ifdef __HIPCC__
// LDS-DMA: 64 lanes x 16 B, global (uniform base + per-lane 32-bit byte offset) -> LDS [lds_dst + lane*16].  Invisible to
// hipcc's s_waitcnt bookkeeping: count completion by hand (vmcnt), then barrier, then read (cdna_hip_programming 5.7).
__device__ __forceinline__ void glds16(const void *base, unsigned voff, unsigned lds_dst) {
    unsigned keep;
    asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %3\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, %2\n\ts_mov_b32 m0, %0"
                 : "=&s"(keep) : "v"(voff), "s"(base), "s"(lds_dst) : "memory");
}
#endif

int sn_pixels_run(cnmfe_ctx *ctx, Patch *P, float *sn_out);
int fast_temporal_run(cnmfe_ctx *ctx, Patch *P, int32_t K, const int64_t *A_colptr, const int32_t *A_rowidx, const float *A_val,
                      int c_order, float *C_raw_out, float *aa_out);
int deconv_bound_run(cnmfe_ctx *ctx, const cnmfe_deconv_opts *opts, float *C_out, float *C_raw_out, float *S_out, float *pars_out, float *sn_out);
int deconv_all_run(cnmfe_ctx *ctx, int32_t K, int64_t T, float *C_raw, int c_order, const cnmfe_deconv_opts *opts,
                   float *C_out, float *S_out, float *pars_out, float *sn_out);
// dff.hpp (deconv.hip)
int df_begin_run(cnmfe_ctx *ctx, int32_t K, int64_t T);
int df_stage_a(cnmfe_ctx *ctx, int32_t Km, const int64_t *cp, const int32_t *ri, const float *va, const int32_t *ind);
int df_project_run(cnmfe_ctx *ctx, int32_t Km, int64_t d, int64_t frame0, int64_t nframes, const float *dY);
int df_add_frames_run(cnmfe_ctx *ctx, int64_t d, int64_t frame0, int64_t nframes, const float *Ybg, int memspace, int32_t Km, const int64_t *cp, const int32_t *ri,
                      const float *va, const int32_t *ind);
int df_chunk_frames(int64_t d, int64_t T, int64_t *nch);
float *df_chunk_buf(cnmfe_ctx *ctx, int64_t d, int64_t nch);
int df_fetch_run(cnmfe_ctx *ctx, double *out);
int df_load_run(cnmfe_ctx *ctx, int32_t K, int64_t T, const double *Yf);
int df_source_check(cnmfe_ctx *ctx, int32_t K, int64_t T, int src);
int df_finish_run(cnmfe_ctx *ctx, const double *inv_norm, double p, int64_t w, const float *C, int c_src, const float *C_raw, int raw_src, float *C_df_out,
                  float *C_raw_df_out, double *Df_out, double *Yf_out);
// demix.hpp (resid.hip): the panels of show_demixed_video, device pointers to nframes x d each (mixed: three such planes), any may be null
struct DemixOut { float *raw, *bg, *signal, *denoised, *residual; unsigned short *mixed; };
int demix_stage(cnmfe_ctx *ctx, Patch *P, int32_t Ksel, const int64_t *cp, const int32_t *ri, const float *va, const int32_t *trow, const float *col);
int demix_kappa(cnmfe_ctx *ctx, Patch *P, const float *b0_block, const float *b0_new);
int demix_launch(cnmfe_ctx *ctx, Patch *P, int32_t Ksel, const float *dCC, int64_t ldc, double mix_scale, int64_t frame0, int64_t stride, int64_t nframes, int64_t j0,
                 int64_t nj, const float *slab, int64_t slab0, const DemixOut &out);
int demix_launch_lowrank(cnmfe_ctx *ctx, Patch *P, int32_t Ksel, const float *dCC, int64_t ldc, double mix_scale, int64_t frame0, int64_t stride, int64_t nframes,
                         const DemixOut &out);
// merge.hpp (deconv.hip)
int trace_source_dev(cnmfe_ctx *ctx, int32_t K, int64_t T, const float *X, int src, const float **dX);   // the K x ceil4(T) device matrix a trace SOURCE names (a host matrix: one counted upload)
int trace_order_stats_run(cnmfe_ctx *ctx, int32_t K, double *out);
int trace_corr_run(cnmfe_ctx *ctx, int32_t K, int64_t T, const float *X, int src, int raw, double *out);
int trace_diff_spikes_run(cnmfe_ctx *ctx, int32_t K, int64_t T, const float *X, int src, float *sn_out, float *S_out);
int trace_tags_run(cnmfe_ctx *ctx, int32_t K, double *out);
int traces_load_run(cnmfe_ctx *ctx, int32_t K, int64_t T, const float *C, const float *C_raw, const float *S, const float *pars, int c_order);
int trace_energy_run(cnmfe_ctx *ctx, int32_t K, int64_t T, const float *X, int src, double *out);
int traces_grow_run(cnmfe_ctx *ctx, int32_t K_new);
int merge_apply_run(cnmfe_ctx *ctx, int32_t ng, const int32_t *gptr, const int32_t *gidx, const double *w, int32_t nkeep, const int32_t *keep,
                    const cnmfe_deconv_opts *opts, float *C_out, float *C_raw_out, float *S_out, float *pars_out, float *sn_out);
int postproc_run(cnmfe_ctx *ctx, int32_t d1, int32_t d2, int32_t K, const int64_t *A_colptr, const int32_t *A_rowidx,
                 const float *A_val, uint8_t *keep);
int fp_circular_run(cnmfe_ctx *ctx, int32_t d1, int32_t d2, int32_t K, const int64_t *A_colptr, const int32_t *A_rowidx, const float *A_val, int32_t *box_out,
                    int64_t *off, float *out, int64_t out_cap, uint8_t *host_col, int out_memspace);                                  // factor.hip (footprint_ops.hpp)
int fp_dilate_run(cnmfe_ctx *ctx, int32_t d1, int32_t d2, int32_t K, const int64_t *A_colptr, const int32_t *A_rowidx, const float *A_val, const uint8_t *se,
                  int32_t se_h, int32_t se_w, int32_t nb, double nrgthr, int32_t *box_out, int64_t *off, uint8_t *out, int64_t out_cap, uint8_t *host_col, int out_memspace);
int fp_trim_run(cnmfe_ctx *ctx, int32_t d1, int32_t d2, int32_t K, const int64_t *A_colptr, const int32_t *A_rowidx, const float *A_val, double thr, int32_t sz,
                int32_t min_pixel, uint8_t *keep, uint8_t *ind_small, uint8_t *host_col, int out_memspace);
int ensure_ymean(cnmfe_ctx *ctx, Patch *P);
// bg_svd.hpp (vproj.hip): the low-rank background model
int bg_svd_fit_run(cnmfe_ctx *ctx, Patch *P, int nb, int32_t K, const int64_t *A_colptr, const int32_t *A_rowidx, const float *A_val, const float *C, int c_order);
int bg_svd_set_run(cnmfe_ctx *ctx, Patch *P, int nb, const double *b, const double *f, const double *b0);
int bg_svd_get_run(cnmfe_ctx *ctx, Patch *P, double *b, double *f, double *b0);
int bg_svd_resid_run(cnmfe_ctx *ctx, Patch *P, float *Ysig_out, int out_memspace);
int sn_video_run(cnmfe_ctx *ctx, Patch *P, int64_t nframes, float *sn_out);
int seed_images_run(cnmfe_ctx *ctx, const SeedSrc &src, const float *psf, int32_t psf_n, int64_t nframes, const double *Q, int32_t M, float sig,
                    float *Cn_out, float *PNR_out, PeelSession *keep = nullptr);   // seed.hpp (deconv.hip)
int peel_open_residual_run(cnmfe_ctx *ctx, Patch *P, int32_t Ksel, const int64_t *A_colptr, const int32_t *A_rowidx, const float *A_val, const float *C, int c_order,
                           const float *psf, int32_t psf_n, float sig, float *Cn_out, float *PNR_out, float *Sn_out, float *Yres_out, int out_memspace);   // peel.hpp (deconv.hip)
int peel_open_lowrank_run(cnmfe_ctx *ctx, Patch *P, int32_t Ksel, const int64_t *A_colptr, const int32_t *A_rowidx, const float *A_val, const float *C, int c_order,
                          const float *psf, int32_t psf_n, float sig, float *Cn_out, float *PNR_out, float *Sn_out, float *Yres_out, int out_memspace);    // peel.hpp (deconv.hip)
int peel_open_run(cnmfe_ctx *ctx, Patch *P, const float *psf, int32_t psf_n, int64_t nframes, const double *Q, int32_t M, float sig,
                  float *Cn_out, float *PNR_out, float *Sn_out);   // peel.hpp (deconv.hip)
int seed_images_ds_run(cnmfe_ctx *ctx, Patch *P, int ssub, int tsub, const float *psf, int32_t psf_n, int64_t nframes, const double *Q, int32_t M, float sig,
                       float *Cn_out, float *PNR_out);   // ds.hpp (deconv.hip)
int peel_open_ds_run(cnmfe_ctx *ctx, Patch *P, int ssub, int tsub, const float *psf, int32_t psf_n, int64_t nframes, const double *Qpre, int32_t Mpre, float sig,
                     float *Cn_out, float *PNR_out, float *Sn_out, float *Yds_out, int out_memspace);   // ds.hpp (deconv.hip)
int peel_open_residual_ds_run(cnmfe_ctx *ctx, Patch *P, int ssub, int tsub, int32_t Ksel, const int64_t *A_colptr, const int32_t *A_rowidx, const float *A_val,
                              const float *C, int c_order, const float *psf, int32_t psf_n, float sig, float *Cn_out, float *PNR_out, float *Sn_out,
                              float *Yds_out, int out_memspace);   // ds.hpp (deconv.hip)
int peel_extract_run(cnmfe_ctx *ctx, Patch *P, int r, int c, int gSiz, double *corr_box, double *ai_box, double *ci_out, double *stats);
int peel_apply_run(cnmfe_ctx *ctx, Patch *P, int r, int c, int gSiz, const double *ai_box, const double *Hai_box2, const double *ci, double sig, double min_pnr,
                   double min_corr, float *PNR_box2, float *Cn_box2);
int spatial_fetch(cnmfe_ctx *ctx, float *A_out, int64_t nnz);
int spatial_fetch_connected(cnmfe_ctx *ctx, int32_t d1, int32_t d2, int32_t K, const int64_t *IND_colptr, const int32_t *IND_rowidx, float *A_out, uint8_t *keep, bool wait = true);
int temporal_early_project(cnmfe_ctx *ctx, int32_t K, const int64_t *IND_colptr, const int32_t *IND_rowidx, int64_t *token);   // factor.hip; *token = 0: declined
int ring_first_run(cnmfe_ctx *ctx, Patch *P, bool *first);
int ring_stats_enqueue(cnmfe_ctx *ctx, Patch *P);                    // after W changed on the stream: count + row 1 to pinned memory, event
int ring_stats_get(cnmfe_ctx *ctx, Patch *P, int *pmax, bool *first); // waits for that event only (falls back to a fresh evaluation)
int center_traces(cnmfe_ctx *ctx, const float *C, int64_t ldc, int32_t K, int64_t T, DevBuf &Cc, DevBuf &Cmean);
int upload_centered(cnmfe_ctx *ctx, DevBuf &stage, const float *C, int32_t K, int64_t T, int order, DevBuf &Cc, DevBuf &Cmean, int64_t *ldc_out);
int ring_side_ahead(cnmfe_ctx *ctx, Patch *P, int32_t K, const HostCSR *csr, const int64_t *A_colptr, const int32_t *A_rowidx, const float *A_val, bool join_now);   // resid.hip: behind a ring fit's solve, on the side stream (option ring_side)
int ctx_side_stream(cnmfe_ctx *ctx);                    // api.hip: the side stream of option fit_side and its two events (created on first use)
int ctx_errflag(cnmfe_ctx *ctx, int **dflag);            // the device error word (allocated and cleared on first use)
int ctx_check_errflag(cnmfe_ctx *ctx);                   // after a stream sync: CNMFE_ESTATE if a kernel raised it (and clears it)
// The context's side stream standing in for the compute stream (options fit_side, bg.hip, and ring_side, resid.hip): between enter() and leave() launches, held-back
// uploads and the profiler's events follow it through cnmfe_ctx::st().  Two ways to start: fork() -- the side stream waits for the compute stream as it stands NOW,
// and leave() makes the compute stream wait for the scope at once; fork_behind() -- it waits for an event recorded EARLIER (ev_ring_solved: a ring fit's solve) and
// leave() only records ev_ring_join: the compute stream waits later, in cnmfe_ctx::ring_side_join().
struct SideScope {
    cnmfe_ctx *ctx; bool inside = false, deferred = false;
    explicit SideScope(cnmfe_ctx *c) : ctx(c) {}
    int fork() {
        int *dErr = nullptr;
        RET(ctx_errflag(ctx, &dErr));                            // (allocated and cleared on the compute stream, before anything can raise it from the other one)
        RET(ctx_side_stream(ctx));
        CK(hipEventRecord(ctx->ev_side_fork, ctx->st()));
        CK(hipStreamWaitEvent(ctx->side_stream, ctx->ev_side_fork, 0));
        return 0;
    }
    // (the caller has the error word in place from before `ev` was recorded, and the side stream exists: the event is one of its set)
    int fork_behind(hipEvent_t ev) { deferred = true; CK(hipStreamWaitEvent(ctx->side_stream, ev, 0)); return 0; }
    int enter() { (void)ctx->st(); std::swap(ctx->stream_, ctx->side_stream); inside = true; return 0; }   // (st(): the compute stream's held-back uploads go out on it)
    int leave() {
        if (!inside) return 0;
        const hipError_t e = hipEventRecord(deferred ? ctx->ev_ring_join : ctx->ev_side_join, ctx->st());     // (st(): the scope's own uploads are sent first)
        std::swap(ctx->stream_, ctx->side_stream); inside = false;
        CK(e);
        if (deferred) { ctx->ring_join_pending = ctx->ring_join_used = true; return 0; }
        CK(hipStreamWaitEvent(ctx->stream_, ctx->ev_side_join, 0));
        return 0;
    }
    // (an error inside the scope: the streams go back, and the compute stream still waits for what was queued)
    ~SideScope() { if (inside) { (void)leave(); if (deferred) (void)ctx->ring_side_join(); } }
};
}  // namespace cnmfe
