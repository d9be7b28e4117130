// Results that outlive the call that computed them (factor.hip, deconv.hip, api.hip): what a deferred spatial update left in a lane's scratch slots, and the tag of
// the temporal projection queued ahead of its consumer.  Plain C++17, no HIP, no engine types, so that tests/kept_results_driver.cpp runs every combination under
// the sanitizers without a GPU.  The buffers stay where they are (cnmfe::LaneState::scr, cnmfe_ctx::EarlyU); the records here say what they hold, and every rule
// that reads a record has ONE copy here ("Lane state and kept results").
#pragma once
#include <cstddef>
#include <cstdint>

namespace cnmfe {
struct Patch;
namespace kept {

// the four scratch slots (LaneState::scr) a kept spatial result lies in: the mask's CSC pattern, the new values, the keep flags of the connectivity kernel.
// Whoever writes one of them calls KeptSpatial::drop() (the values go) or drop_pattern() (only the pattern or the flags go) first.
enum Slot { SCR_COLPTR = 0, SCR_EROW = 1, SCR_AVAL = 6, SCR_KEEP = 14 };

// What the last cnmfe_update_spatial of a lane left in that lane's slots.  nnz: values in SCR_AVAL (-1: none); patch, K, gen: the patch, the number of columns and
// the context-wide count (cnmfe_ctx::spatial_gen) of that update; pattern: its mask still lies in SCR_COLPTR / SCR_EROW; flags: its keep flags lie in SCR_KEEP
// (the connected fetch has run since, and the pattern is still in place).
struct KeptSpatial {
    int64_t nnz = -1; const Patch *patch = nullptr; int32_t K = 0; int64_t gen = 0; bool pattern = false, flags = false;
    void record(int64_t nnz_, const Patch *P, int32_t K_, int64_t gen_) { nnz = nnz_; patch = P; K = K_; gen = gen_; pattern = nnz_ > 0; flags = false; }
    void flags_written() { flags = pattern; }                // (the connectivity kernel of the connected fetch)
    void drop() { *this = KeptSpatial(); }                   // SCR_AVAL changes hands: nothing of the result is left
    void drop_pattern() { pattern = flags = false; }         // SCR_COLPTR / SCR_EROW / SCR_KEEP change hands, the values stay
    void patch_gone() { patch = nullptr; }                   // a patch was created or replaced: the record may name the one that went (the values can still be fetched)
    bool fetchable(int64_t n) const { return nnz >= 0 && n == nnz; }                               // cnmfe_update_spatial_fetch[_async]
    bool fetchable_connected(int64_t n) const { return fetchable(n) && (n == 0 || pattern); }      // ..._fetch_connected[_async]: the kernel reads the pattern
};

// the options that select the kernel of the temporal projection (vproj.hip), with their defaults where they are read: common.hpp, proj_opts
struct ProjOpts {
    int64_t i8 = 1, i8_planes = 3, tiled = 1;
    bool operator==(const ProjOpts &o) const { return i8 == o.i8 && i8_planes == o.i8_planes && tiled == o.tiled; }
};

// ---- the hand-over: U = B' Yc queued behind the connectivity kernel (option temporal_early; include/cnmfe.h, cnmfe_temporal_early_project) ----------------------
// The tag of the queued projection: what it was computed for.  token: handed to the caller; claimed: the token the caller gave back (its A IS that spatial result).
struct EarlyTag {
    bool valid = false; int64_t token = 0, claimed = 0;
    const Patch *P = nullptr; int32_t K = 0; int64_t ldc = 0, T = 0, spatial_gen = 0, request_gen = 0;   // request_gen (ResidualState::gen): W, b0 and the video only change in front of a new residual request
    ProjOpts proj;
};
// a temporal update as the tag is compared with it (temporal_run, non-job path)
struct TakeRequest {
    int64_t mode;                                            // option temporal_early
    const Patch *P; int32_t K; int64_t ldc, T, spatial_gen, request_gen, nnz;
    bool is_virtual, src_full, one_lane, terms_match;        // the patch's residual is a recorded request of cnmfe_residual; lanes = 1; rplan::terms_match_stride at ldc
    ProjOpts proj;
};
// may the temporal update take the projection queued ahead?  (the caller has checked tag.valid and consumes the tag either way)
inline bool early_takes(const EarlyTag &E, const TakeRequest &q) {
    return (q.mode == 1 || q.mode == 2) && E.claimed == E.token && E.P == q.P && E.K == q.K && E.ldc == q.ldc && E.T == q.T && E.spatial_gen == q.spatial_gen
           && E.request_gen == q.request_gen && q.nnz > 0 && q.is_virtual && q.src_full && q.one_lane
           && q.terms_match                                  // (the term would be folded into Ysig: no virtual residual then)
           && E.proj == q.proj;
}
// a request to queue the projection (temporal_early_project); the patch's properties are those of kept.patch (false without one)
struct ServeRequest {
    int64_t mode; bool one_lane;
    int32_t K; int64_t nnz, spatial_gen;
    bool patch_is_fov, is_virtual, src_full;
};
enum Serve { SERVE_OFF = 0, SERVE_DECLINED = 1, SERVE_YES = 2 };   // off: not counted; declined: counter temporal_early_declined
inline Serve early_serves(const KeptSpatial &k, const ServeRequest &q) {
    if ((q.mode != 1 && q.mode != 2) || !q.one_lane) return SERVE_OFF;
    if (!k.patch || k.K != q.K || q.nnz == 0 || k.nnz != q.nnz || !k.flags || k.gen != q.spatial_gen
        || !q.patch_is_fov || !q.is_virtual || !q.src_full) return SERVE_DECLINED;
    return SERVE_YES;
}

// ---- option ring_side: the W A tables of a residual request on the side stream, behind the event of the last ring fit's solve (resid.hip, residual_run) ----------
// solve_marked: ResidualState -- the patch's W is final behind that event and nothing has invalidated since (the outlier branch and bg_ssub's fits do not mark);
// foreign / tables_only / want_out: the request of a low-resolution patch, or one whose Ysig is read at once; recorded: the plan only records the request or
// pends its term (the virtual request of the steady state) -- a sweep reads the tables on the compute stream right away
struct RingSideRequest { int64_t mode; bool one_lane; size_t npatches; bool solve_marked, has_ac, foreign, tables_only, want_out, recorded; };
inline bool ring_side_applies(const RingSideRequest &q) {
    return (q.mode == 1 || q.mode == 2) && q.one_lane && q.npatches == 1 && q.solve_marked && q.has_ac && !q.foreign && !q.tables_only && !q.want_out && q.recorded;
}

}  // namespace kept
}  // namespace cnmfe
