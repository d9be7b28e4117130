// Stand-alone driver of cnmf_e_amd/csrc/residual_plan.hpp for tests/test_residual_plan.py: reads one command per line from a case file, prints one line of
// integers per command.  Built with the host compiler and the address / undefined-behaviour sanitizers; no GPU, no HIP.
//   plan   form source buffer  qsource has_ac want_out outbuf tables_only  delta lazy virt ssub_virtual samples   -> action reuse virt_new tables
//   kernel radius full_ring has_ac can_defer  variant lazy defer                                                   -> variant special small_special TR TC defer_term sweep_ac
//   terms  has_pending  pend_ac pend_ldc pend_K  res_ac res_ldc res_K  ldc K                                       -> match_stride projectable foldable overflow_possible
// legacy_plan / legacy_kernel / legacy_terms take the same arguments and answer with the expressions of resid.hip, ssub.hip and factor.hip as they stood before the
// rules moved into the header (copied verbatim; the small structs below stand in for the patch and the context they were written against).
#include "../cnmf_e_amd/csrc/residual_plan.hpp"
#include <cstdio>
#include <cstring>
#include <fstream>
#include <string>
using namespace cnmfe;
using namespace cnmfe::rplan;

namespace legacy {
struct Buf { const void *p; };
struct Patch {
    bool ysig_valid, ysig_virtual; int res_kind; Buf ysig; int64_t d_b, T; int radius;
    bool pend, pend_ac, res_ac; int64_t pend_ldc, res_ldc; int32_t pend_K, res_K;
};
struct Ctx {
    int64_t delta, lazy, defer, virt, sv, variant;
    int64_t opt(const char *n, int64_t) const {
        return !strcmp(n, "r1_delta") ? delta : !strcmp(n, "r1_lazy") ? lazy : !strcmp(n, "r1_defer") ? defer : !strcmp(n, "r1_virtual") ? virt : !strcmp(n, "ssub_virtual") ? sv : variant;
    }
};
constexpr int ARC_TR = 16, ARC_TC = 32, DUO_T = 32, TERM_KMAX = 8192;
constexpr int64_t FOLD_MAX_PAIRS = int64_t(1) << 16;
static void tile_shape(int variant, int &TR, int &TC) {
    TR = 32; TC = 16;                                     // variant 10
    if (variant == 11) { TR = ARC_TR; TC = ARC_TC; }
    else if (variant == 14) { TR = DUO_T; TC = DUO_T; }
}

// residual_run: 0 only pend, 1 pend and fold, 2 record, 3 sweep
static void full(const Ctx *ctx, const Patch *P, const void *outbuf, const void *Ysig_out, int tables_only, int out[4]) {
    const bool delta = !outbuf && P->ysig_valid && P->res_kind == 1 && (P->ysig.p || P->ysig_virtual) && ctx->opt("r1_delta", 1) != 0;
    out[1] = delta; out[2] = 0; out[3] = tables_only;
    if (delta) {
        if (ctx->opt("r1_lazy", 1) != 0 && !Ysig_out) { out[0] = 0; return; }
        out[0] = 1; return;
    }
    if (!outbuf && !Ysig_out && ctx->opt("r1_virtual", 1) != 0 && ctx->opt("r1_lazy", 1) != 0 && ctx->opt("r1_delta", 1) != 0) { out[0] = 2; out[2] = 1; return; }
    out[0] = 3;
}
static void ssub(const Ctx *ctx, const Patch *M, const void *Ysig_out, int out[4]) {
    const bool lazy = ctx->opt("r1_delta", 1) != 0;
    const bool reuse = M->ysig_valid && M->res_kind == 2 && (M->ysig.p || M->ysig_virtual) && lazy;
    const int64_t sv = ctx->opt("ssub_virtual", 1);
    const bool virt_new = !reuse && !Ysig_out && lazy && (sv >= 2 || (sv == 1 && (double)M->d_b * (double)M->T >= 5e8)) && ctx->opt("r1_virtual", 1) != 0 && ctx->opt("r1_lazy", 1) != 0;
    const bool tables = reuse || virt_new;
    out[1] = reuse; out[2] = virt_new; out[3] = tables;
    if (tables) {
        if (virt_new) { out[0] = 2; return; }
        if (ctx->opt("r1_lazy", 1) == 0 || Ysig_out) { out[0] = 1; return; }
        out[0] = 0; return;
    }
    out[0] = 3;
}
static void kernel(const Ctx *ctx, const Patch *P, bool full_ring, bool has_ac, bool can_defer, int out[7]) {
    int variant = (int)ctx->opt("r1_variant", 14);
    const int h = P->radius;
    if (variant >= 0 && variant != 10 && variant != 11 && variant != 14) variant = 14;
    const bool defer_term = has_ac && variant == 14 && h == 15 && full_ring && can_defer && ctx->opt("r1_lazy", 1) != 0 && ctx->opt("r1_defer", 1) != 0;
    const bool sweep_ac = has_ac && !defer_term;
    if (variant == 14 && (sweep_ac || h != 15)) variant = 11;   // duo roles (resid_duo.hpp): radius 15, no footprint term inside the sweep
    if (h == 18 && variant >= 11) variant = 10;               // arc kernels: radius 15 only (ds_read immediates)
    const bool small_special = full_ring && (h == 5 || h == 6 || h == 8 || h == 9) && variant >= 0;
    if (small_special) variant = 10;
    const bool special = (full_ring && (h == 15 || h == 18) && variant >= 0) || small_special;
    int TR = 16, TC = 16;
    if (special) tile_shape(variant, TR, TC);
    out[0] = variant; out[1] = special; out[2] = small_special; out[3] = TR; out[4] = TC; out[5] = defer_term; out[6] = sweep_ac;
}
static void terms(const Patch *P, int64_t ldc, int32_t K, int out[4]) {
    const int64_t ldu = ldc;
    out[0] = !(P->pend && (P->pend_ldc != ldc || (P->res_ac && P->res_ldc != ldc)));
    out[1] = !P->pend || !((P->pend_ac && (P->pend_K > TERM_KMAX || P->pend_ldc != ldu)) || (P->res_ac && (P->res_K > TERM_KMAX || P->res_ldc != ldu)));
    out[2] = [&]() {
        if (!P->pend) return true;
        if (P->pend_ac && (P->pend_ldc != ldc || (int64_t)P->pend_K * K > FOLD_MAX_PAIRS)) return false;
        if (P->res_ac && (P->res_ldc != ldc || (int64_t)P->res_K * K > FOLD_MAX_PAIRS)) return false;
        return true;
    }();
    const bool term_applied = P->pend;
    out[3] = term_applied && ((P->pend_ac && P->pend_K > 512) || (P->res_ac && P->res_K > 512));
}
}  // namespace legacy

static void put(const int *v, int n) { for (int i = 0; i < n; ++i) std::printf(i ? " %d" : "%d", v[i]); std::printf("\n"); }

int main(int argc, char **argv) {
    if (argc != 2) return 2;
    std::ifstream in(argv[1]);
    std::string cmd;
    static const char dummy = 0;
    while (in >> cmd) {
        const bool old = cmd.rfind("legacy_", 0) == 0;
        if (old) cmd = cmd.substr(7);
        if (cmd == "plan") {
            int form, source, buffer, qsource, has_ac, want, outbuf, tables_only; long long delta, lazy, virt, sv, samples;
            in >> form >> source >> buffer >> qsource >> has_ac >> want >> outbuf >> tables_only >> delta >> lazy >> virt >> sv >> samples;
            int out[4];
            if (old) {
                legacy::Patch P{}; legacy::Ctx c{delta, lazy, 1, virt, sv, 14};
                P.ysig_valid = form != NONE; P.ysig_virtual = form == VIRTUAL; P.res_kind = source; P.ysig.p = buffer ? &dummy : nullptr; P.d_b = samples; P.T = 1;
                if (qsource == SRC_SSUB) legacy::ssub(&c, &P, want ? &dummy : nullptr, out);
                else legacy::full(&c, &P, outbuf ? &dummy : nullptr, want ? &dummy : nullptr, tables_only, out);
            } else {
                ResidualOpts o; o.delta = delta; o.lazy = lazy; o.virt = virt; o.ssub_virtual = sv;
                const Plan p = residual_plan(View{(Form)form, source, buffer != 0}, Request{qsource, has_ac != 0, want != 0, outbuf != 0, tables_only != 0, (double)samples}, o);
                out[0] = p.action; out[1] = p.reuse; out[2] = p.virt_new; out[3] = p.tables;
            }
            put(out, 4);
        } else if (cmd == "kernel") {
            int radius, full_ring, has_ac, can_defer; long long variant, lazy, defer;
            in >> radius >> full_ring >> has_ac >> can_defer >> variant >> lazy >> defer;
            int out[7];
            if (old) {
                legacy::Patch P{}; P.radius = radius; legacy::Ctx c{1, lazy, defer, 1, 1, variant};
                legacy::kernel(&c, &P, full_ring != 0, has_ac != 0, can_defer != 0, out);
            } else {
                ResidualOpts o; o.variant = variant; o.lazy = lazy; o.defer = defer;
                const R1Kernel k = r1_kernel_plan(o, radius, full_ring != 0, has_ac != 0, can_defer != 0);
                out[0] = k.variant; out[1] = k.special; out[2] = k.small_special; out[3] = k.TR; out[4] = k.TC; out[5] = k.defer_term; out[6] = k.sweep_ac;
            }
            put(out, 7);
        } else if (cmd == "terms") {
            int has_pending, pend_ac, res_ac; long long pend_ldc, pend_K, res_ldc, res_K, ldc, K;
            in >> has_pending >> pend_ac >> pend_ldc >> pend_K >> res_ac >> res_ldc >> res_K >> ldc >> K;
            int out[4];
            if (old) {
                legacy::Patch P{}; P.pend = has_pending; P.pend_ac = pend_ac; P.pend_ldc = pend_ldc; P.pend_K = (int32_t)pend_K; P.res_ac = res_ac; P.res_ldc = res_ldc; P.res_K = (int32_t)res_K;
                legacy::terms(&P, ldc, (int32_t)K, out);
            } else {
                const TermsView t{has_pending != 0, TermView{res_ac != 0, res_ldc, (int32_t)res_K}, TermView{pend_ac != 0, pend_ldc, (int32_t)pend_K}};
                out[0] = terms_match_stride(t, ldc); out[1] = term_projectable(t, ldc); out[2] = term_foldable_spatial(t, (int32_t)K, ldc);
                out[3] = t.has_pending && term_overflow_possible(t);
            }
            put(out, 4);
        } else
            return 3;
        if (!in) return 4;
    }
    return 0;
}
