// The host rules of the residual (resid.hip, ssub.hip, the residual parts of factor.hip): what a request does to the state kept beside Ysig, which kernel the
// sweep takes, and whether a footprint term can go through a projection.  Plain C++17, no HIP, no engine types, so that tests/residual_plan_driver.cpp runs every
// combination under the sanitizers without a GPU.  Every rule has ONE copy here; Patch::residual (common.hpp) holds the state these rules read.
#pragma once
#include <cstdint>

namespace cnmfe {
namespace rplan {

// ---- the state beside Ysig, as the rules see it -----------------------------------------------------------------------------------------------------------
enum Form { NONE = 0, VIRTUAL = 1, RESIDENT = 2 };        // no residual | a recorded request (no sweep has run) | Ysig itself lies in the patch's buffer
enum Source { SRC_NONE = 0, SRC_FULL = 1, SRC_SSUB = 2, SRC_LOWRANK = 3 }; // who wrote it: cnmfe_residual | cnmfe_residual_ssub | cnmfe_residual_lowrank
struct TermView { bool ac; int64_t ldc; int32_t K; };     // a footprint term: has footprints at all, row stride of its centred traces, number of traces
struct TermsView { bool has_pending; TermView applied, pending; };
struct View { Form form; int source; bool buffer; };      // buffer: the patch's Ysig buffer is allocated

// the options of the residual, read once per call (resid.hip, residual_opts: the only place that names them and their defaults)
struct ResidualOpts { int64_t delta = 1, lazy = 1, defer = 1, virt = 1, ssub_virtual = 1, variant = 14, probe = 0; };

// ---- what a request does ------------------------------------------------------------------------------------------------------------------------------------
//   PendOnly     the residual under the current video, W and b0 exists (swept or recorded): the new footprint term only pends beside it
//   PendAndFold  the same, and the term is folded into Ysig now (somebody reads Ysig: an output buffer, or r1_lazy = 0)
//   Record       nothing valid is kept and nobody reads Ysig: the request is recorded (VIRTUAL), its term pends
//   Sweep        the ring sweep runs (cnmfe_residual: of the patch; cnmfe_residual_ssub: of the low-resolution patch, then the upsample)
enum Action { PendOnly = 0, PendAndFold = 1, Record = 2, Sweep = 3 };
struct Request { int source; bool has_ac, want_out, outbuf, tables_only; double samples; };   // outbuf: the sweep goes into a foreign buffer and the patch's state stays
                                                                                              // as it is; tables_only: only W A and the centred traces are wanted
                                                                                              // (both: the low-resolution patch of a cnmfe_residual_ssub); samples: d_b T
// reuse: the kept residual serves (PendOnly / PendAndFold); virt_new: Record; tables: the low-resolution patch builds its tables only (no sweep there)
struct Plan { Action action; bool reuse, virt_new, tables; };
constexpr double SSUB_VIRTUAL_SAMPLES = 5e8;              // ssub_virtual = 1 records on patches of at least this many samples
inline Plan residual_plan(const View &v, const Request &q, const ResidualOpts &o) {
    const bool ssub = q.source == SRC_SSUB;
    const bool foreign = !ssub && q.outbuf;                 // (cnmfe_residual_ssub always works on the patch's own state)
    const bool kept = v.form != NONE && v.source == q.source && (v.buffer || v.form == VIRTUAL);
    const bool incremental = o.delta != 0;                  // (r1_delta = 0: every request starts from the video)
    Plan p{Sweep, false, false, false};
    p.reuse = kept && incremental && !foreign;
    const bool size_ok = !ssub || o.ssub_virtual >= 2 || (o.ssub_virtual == 1 && q.samples >= SSUB_VIRTUAL_SAMPLES);
    p.virt_new = !p.reuse && !foreign && !q.want_out && incremental && o.lazy != 0 && o.virt != 0 && size_ok;
    p.tables = ssub ? (p.reuse || p.virt_new) : q.tables_only;
    if (p.reuse) p.action = (o.lazy != 0 && !q.want_out) ? PendOnly : PendAndFold;
    else if (p.virt_new) p.action = Record;
    return p;
}

// ---- the low-rank background (background_model = 'svd', bg_svd.hpp) ------------------------------------------------------------------------------------------
// Its residual Yc + (Ymean - b0) - b f is always RESIDENT, carries no footprint term (nothing applied, nothing pending) and is never recorded: the sweep-free form
// would be a rank-nb correction of the projections and is not built.  A fit, a transplant of b, f, b0 and an upload of the video invalidate it; a request that finds
// it still valid has nothing to do.  A ring request (SRC_FULL / SRC_SSUB) never reuses it and it never reuses theirs: residual_plan's `kept` compares the sources.
struct LowrankPlan { bool sweep; };
inline LowrankPlan lowrank_plan(const View &v) { return {!(v.form == RESIDENT && v.source == SRC_LOWRANK && v.buffer)}; }
// compute_RSS and reconstruct_background are built on the ring's W: they serve the residual of cnmfe_residual only
inline bool serves_ring_readers(int source) { return source == SRC_FULL; }

// ---- the kernel of the sweep --------------------------------------------------------------------------------------------------------------------------------
// variant: 14 duo-role kernel (radius 15, no footprint term inside the sweep), 11 arc kernel (radius 15), 10 LDS-DMA kernel (radius 15 / 18 and the low-resolution
// rings 5, 6, 8, 9 of bg_ssub = 2, 3), -1 the generic kernel; special: a compile-time kernel of the full ring runs, on TR x TC tiles (resid.hip asserts these
// against the kernels' own constants).  defer_term: the sweep runs without the footprint term and the term pends (r1_defer); sweep_ac: the term goes through the sweep
struct R1Kernel { int variant; bool special, small_special; int TR, TC; bool defer_term, sweep_ac; };
constexpr int R1_DMA_TR = 32, R1_DMA_TC = 16, R1_ARC_TR = 16, R1_ARC_TC = 32, R1_DUO_T = 32, R1_GEN_T = 16;
inline R1Kernel r1_kernel_plan(const ResidualOpts &o, int radius, bool full_ring, bool has_ac, bool can_defer) {
    R1Kernel k{};
    const int h = radius;
    int variant = (int)o.variant;
    if (variant >= 0 && variant != 10 && variant != 11 && variant != 14) variant = 14;
    k.defer_term = has_ac && variant == 14 && h == 15 && full_ring && can_defer && o.lazy != 0 && o.defer != 0;
    k.sweep_ac = has_ac && !k.defer_term;
    if (variant == 14 && (k.sweep_ac || h != 15)) variant = 11;   // duo roles (resid_duo.hpp): radius 15, no footprint term inside the sweep
    if (h == 18 && variant >= 11) variant = 10;                   // arc kernels: radius 15 only (ds_read immediates)
    k.small_special = full_ring && (h == 5 || h == 6 || h == 8 || h == 9) && variant >= 0;
    if (k.small_special) variant = 10;
    k.special = (full_ring && (h == 15 || h == 18) && variant >= 0) || k.small_special;
    k.variant = variant;
    k.TR = k.TC = R1_GEN_T;
    if (k.special) {
        k.TR = R1_DMA_TR; k.TC = R1_DMA_TC;
        if (variant == 11) { k.TR = R1_ARC_TR; k.TC = R1_ARC_TC; }
        else if (variant == 14) { k.TR = k.TC = R1_DUO_T; }
    }
    return k;
}

// ---- can the terms go through a projection instead of a pass over Ysig? ------------------------------------------------------------------------------------
constexpr int TERM_KMAX = 8192;                           // trace ids the bitmap of k_term_project covers
constexpr int TERM_LIST = 512;                            // traces near one footprint its list holds
constexpr int64_t FOLD_MAX_PAIRS = int64_t(1) << 16;      // K_term x K inner products of the spatial fold (k_cross_gram)
// every term that takes part has the row stride ldc (the pending one always takes part, the applied one when it has footprints)
inline bool terms_match_stride(const TermsView &t, int64_t ldc) {
    return !t.has_pending || (t.pending.ldc == ldc && !(t.applied.ac && t.applied.ldc != ldc));
}
// the temporal projection (k_term_project) can take both terms in: trace ids within its bitmap, rows of stride ldu
inline bool term_projectable(const TermsView &t, int64_t ldu) {
    auto ok = [&](const TermView &x) { return !x.ac || (x.K <= TERM_KMAX && x.ldc == ldu); };
    return !t.has_pending || (ok(t.pending) && ok(t.applied));
}
// the spatial projection onto K traces of stride ldc can (k_cross_gram + k_term_fold_spatial)
inline bool term_foldable_spatial(const TermsView &t, int32_t K, int64_t ldc) {
    auto ok = [&](const TermView &x) { return !x.ac || (x.ldc == ldc && (int64_t)x.K * K <= FOLD_MAX_PAIRS); };
    return !t.has_pending || (ok(t.pending) && ok(t.applied));
}
// k_term_project may meet more traces near one footprint than its list holds: only a term with more traces than that can
inline bool term_overflow_possible(const TermsView &t) {
    return t.has_pending && ((t.pending.ac && t.pending.K > TERM_LIST) || (t.applied.ac && t.applied.K > TERM_LIST));
}

}  // namespace rplan
}  // namespace cnmfe
