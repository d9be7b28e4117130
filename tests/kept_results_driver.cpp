// Host-only driver of cnmf_e_amd/csrc/kept_results.hpp for tests/test_kept_results.py: reads one case per line from the file named on the command line (a
// command and integers), prints one line of integers per case.  Built with the host compiler under the address and undefined-behaviour sanitizers; no HIP.
// The legacy_* commands are the boolean expressions of factor.hip and api.hip as they stood before the rules moved into the header, on the loose fields the
// context had then (spatial_nnz, spatial_patch, spatial_K, spatial_gen, conn_gen); `lanestate` moves a LaneState-shaped struct of stub buffers.
#include "../cnmf_e_amd/csrc/kept_results.hpp"

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <sstream>
#include <string>
#include <utility>
#include <vector>
#include <fstream>

namespace cnmfe { struct Patch { int id; }; }
using namespace cnmfe;
using namespace cnmfe::kept;

static Patch g_p0{0}, g_p1{1};

// ---- early_takes: mode, then one flag per field (1: the tag's field equals the request's), nnz, the four request properties, the three options -----------------
struct TakeCase { long long mode; int claimed, P, K, ldc, T, sgen, rgen; long long nnz; int virt, full, one_lane, terms, i8, planes, tiled; };
static TakeCase take_case(const std::vector<long long> &a) {
    return {a[0], (int)a[1], (int)a[2], (int)a[3], (int)a[4], (int)a[5], (int)a[6], (int)a[7], a[8], (int)a[9], (int)a[10], (int)a[11], (int)a[12], (int)a[13], (int)a[14], (int)a[15]};
}
static int run_takes(const TakeCase &c) {
    EarlyTag E; E.valid = true; E.token = 7; E.claimed = c.claimed ? 7 : 0;
    E.P = &g_p0; E.K = 4; E.ldc = 64; E.T = 61; E.spatial_gen = 3; E.request_gen = 9; E.proj = ProjOpts{1, 3, 1};
    TakeRequest q{c.mode, c.P ? &g_p0 : &g_p1, c.K ? 4 : 5, c.ldc ? 64 : 68, c.T ? 61 : 62, c.sgen ? 3 : 4, c.rgen ? 9 : 10, c.nnz,
                  c.virt != 0, c.full != 0, c.one_lane != 0, c.terms != 0, ProjOpts{c.i8 ? 1 : 0, c.planes ? 3 : 4, c.tiled ? 1 : 0}};
    return early_takes(E, q);
}
static int legacy_takes(const TakeCase &c) {
    // factor.hip, temporal_run before the change: E.* the tag, the right-hand sides the call's own values
    struct { long long claimed, token; const Patch *P; int K; long long ldc, T, spatial_gen, request_gen, proj_i8, proj_i8_planes, proj_tiled; } E{c.claimed ? 7 : 0, 7, &g_p0, 4, 64, 61, 3, 9, 1, 3, 1};
    const long long te_mode = c.mode, ldc = c.ldc ? 64 : 68, T = c.T ? 61 : 62, ctx_spatial_gen = c.sgen ? 3 : 4, P_residual_gen = c.rgen ? 9 : 10, nnz = c.nnz;
    const Patch *P = c.P ? &g_p0 : &g_p1; const int K = c.K ? 4 : 5;
    const bool is_virtual = c.virt != 0, source_full = c.full != 0, lanes_empty = c.one_lane != 0, terms_match_stride = c.terms != 0;
    const long long opt_i8 = c.i8 ? 1 : 0, opt_planes = c.planes ? 3 : 4, opt_tiled = c.tiled ? 1 : 0;
    return (te_mode == 1 || te_mode == 2) && E.claimed == E.token && E.P == P && E.K == K && E.ldc == ldc && E.T == T && E.spatial_gen == ctx_spatial_gen
           && E.request_gen == P_residual_gen && nnz > 0 && is_virtual && source_full && lanes_empty
           && terms_match_stride
           && E.proj_i8 == opt_i8 && E.proj_i8_planes == opt_planes && E.proj_tiled == opt_tiled;
}

// ---- early_serves: mode, one_lane, has_patch, K equal, nnz of the request, record's nnz equal, keep flags in place, generation equal, fov, virtual, full -------
struct ServeCase { long long mode; int one_lane, has_patch, K; long long nnz; int nnz_eq, flags, gen_eq, fov, virt, full; };
static ServeCase serve_case(const std::vector<long long> &a) {
    return {a[0], (int)a[1], (int)a[2], (int)a[3], a[4], (int)a[5], (int)a[6], (int)a[7], (int)a[8], (int)a[9], (int)a[10]};
}
static int run_serves(const ServeCase &c) {
    KeptSpatial k;
    k.record(c.nnz_eq ? c.nnz : c.nnz + 1, &g_p0, c.K ? 4 : 5, 3);
    if (c.flags) { k.pattern = true; k.flags_written(); }      // (pattern forced: the product also holds nnz = 0, where no mask is recorded)
    if (!c.has_patch) k.patch_gone();
    const bool has = k.patch != nullptr;
    return early_serves(k, {c.mode, c.one_lane != 0, 4, c.nnz, c.gen_eq ? 3 : 4, has && c.fov, has && c.virt, has && c.full});
}
static int legacy_serves(const ServeCase &c) {
    // factor.hip, temporal_early_project before the change: 0 returned without counting, 1 declined (counted), 2 goes on
    const long long mode = c.mode, nnz = c.nnz, spatial_nnz = c.nnz_eq ? c.nnz : c.nnz + 1, spatial_gen = c.gen_eq ? 3 : 4, conn_gen = c.flags ? 3 : -1;
    const bool lanes_empty = c.one_lane != 0;
    const Patch *P = c.has_patch ? &g_p0 : nullptr; const int spatial_K = c.K ? 4 : 5, K = 4;
    const bool P_is_fov = c.fov != 0, P_virtual = c.virt != 0, P_full = c.full != 0;
    if ((mode != 1 && mode != 2) || !lanes_empty) return 0;
    if (!P || spatial_K != K || nnz == 0 || spatial_nnz != nnz || conn_gen != spatial_gen
        || !P_is_fov || !P_virtual || !P_full) return 1;
    return 2;
}

// ---- KeptSpatial transitions: a sequence of operations on a fresh record, then what a fetch of 5 values, of 0 values and a hand-over request see --------------
//   1 spatial update of 5 values   2 spatial update of 0 values   3 connected fetch of 5 values (runs its kernel only when its guard lets it)
//   4 drop (a call took the value slot)   5 drop_pattern (a call took the pattern slots)   6 a patch was created or replaced
static void run_kept(const std::vector<long long> &ops, bool legacy) {
    KeptSpatial k; long long ctx_gen = 0;
    // the loose fields of the parent: a call that reused a slot set conn_gen = -1 and nothing else
    long long spatial_nnz = -1, spatial_gen = 0, conn_gen = -1; const Patch *spatial_patch = nullptr;
    for (long long op : ops) {
        if (op == 0) continue;
        if (!legacy) {
            if (op == 1 || op == 2) { k.drop(); ++ctx_gen; k.record(op == 1 ? 5 : 0, &g_p0, 4, ctx_gen); }
            else if (op == 3) { if (k.fetchable_connected(5)) k.flags_written(); }
            else if (op == 4) k.drop();
            else if (op == 5) k.drop_pattern();
            else if (op == 6) k.patch_gone();
        } else {
            if (op == 1 || op == 2) { spatial_nnz = op == 1 ? 5 : 0; ++spatial_gen; spatial_patch = &g_p0; conn_gen = -1; }
            else if (op == 3) { if (!(spatial_nnz < 0 || 5 != spatial_nnz)) conn_gen = spatial_gen; }
            else if (op == 4 || op == 5) conn_gen = -1;
            else if (op == 6) spatial_patch = nullptr;
        }
    }
    if (!legacy) printf("%d %d %d %d %d\n", (int)k.fetchable(5), (int)k.fetchable_connected(5), (int)k.fetchable(0), (int)k.fetchable_connected(0),
                        (int)(k.patch != nullptr && k.flags && k.gen == ctx_gen));
    else printf("%d %d %d %d %d\n", (int)!(spatial_nnz < 0 || 5 != spatial_nnz), (int)!(spatial_nnz < 0 || 5 != spatial_nnz), (int)!(spatial_nnz < 0 || 0 != spatial_nnz),
                (int)!(spatial_nnz < 0 || 0 != spatial_nnz), (int)(spatial_patch != nullptr && conn_gen == spatial_gen));
}

// ---- a LaneState-shaped struct of stub buffers: the move operations of DevBuf / PinArena on host memory ----------------------------------------------------
static int g_live = 0;                                     // allocations alive
struct StubBuf {
    char *p = nullptr; size_t cap = 0;
    StubBuf() = default;
    StubBuf(const StubBuf &) = delete; StubBuf &operator=(const StubBuf &) = delete;
    StubBuf(StubBuf &&o) noexcept : p(o.p), cap(o.cap) { o.p = nullptr; o.cap = 0; }
    StubBuf &operator=(StubBuf &&o) noexcept {
        if (this != &o) { if (p) { delete[] p; --g_live; } p = o.p; cap = o.cap; o.p = nullptr; o.cap = 0; }
        return *this;
    }
    void ensure(size_t n) { if (n <= cap) return; if (p) { delete[] p; --g_live; } p = new char[n]; cap = n; ++g_live; memset(p, (int)(n & 0x7f), n); }
    ~StubBuf() { if (p) { delete[] p; --g_live; } }
};
struct StubArenaFields { char *p = nullptr; size_t cap = 0, off = 0; int half = 0; int *ev[2] = {nullptr, nullptr}; bool ev_set[2] = {false, false}; };
struct StubArena : StubArenaFields {
    StubArena() = default;
    StubArena(const StubArena &) = delete; StubArena &operator=(const StubArena &) = delete;
    StubArena(StubArena &&o) noexcept : StubArenaFields(o) { static_cast<StubArenaFields &>(o) = StubArenaFields(); }
    StubArena &operator=(StubArena &&o) noexcept {
        if (this != &o) { release(); static_cast<StubArenaFields &>(*this) = o; static_cast<StubArenaFields &>(o) = StubArenaFields(); }
        return *this;
    }
    void init(size_t n) { p = new char[n]; cap = n; ++g_live; for (int i = 0; i < 2; ++i) { ev[i] = new int(i); ++g_live; } }
    void release() { if (p) { delete[] p; --g_live; } for (int i = 0; i < 2; ++i) if (ev[i]) { delete ev[i]; --g_live; } static_cast<StubArenaFields &>(*this) = StubArenaFields(); }
    ~StubArena() { release(); }
};
struct StubScratch { StubBuf pv, pw, list; };
struct StubLane {
    void *stream_ = nullptr; int npseg = 0; StubArena pin; StubBuf vp[4]; long long last_ldc = 0; StubBuf bf, tmp[3], scr[24]; StubScratch dscr; KeptSpatial kept;
    StubLane() = default;
    StubLane(StubLane &&) = default; StubLane &operator=(StubLane &&) = default;
};
static void fill(StubLane &L, int tag) {
    static int streams[8];
    L.stream_ = &streams[tag]; L.npseg = tag; L.pin.init(64 + tag); L.last_ldc = 100 + tag; L.bf.ensure(10 + tag);
    for (int i = 0; i < 4; ++i) L.vp[i].ensure(20 + tag + i);
    for (int i = 0; i < 24; i += 2) L.scr[i].ensure(30 + tag + i);              // (every second slot: a lane's slots are not all in use)
    L.tmp[1].ensure(7); L.dscr.pw.ensure(40 + tag); L.kept.record(5 + tag, &g_p0, 4, tag);
}
static long long sig(const StubLane &L) {                  // what a lane holds, as one number
    long long s = L.npseg + 3 * L.last_ldc + 5 * (long long)L.pin.cap + 7 * (long long)L.bf.cap + 11 * L.kept.nnz + (L.pin.ev[1] ? 13 * *L.pin.ev[1] : 0);
    for (int i = 0; i < 4; ++i) s += 17 * (long long)L.vp[i].cap;
    for (int i = 0; i < 24; ++i) s += (19 + i) * (long long)L.scr[i].cap;
    return s + 23 * (long long)L.dscr.pw.cap + 29 * (long long)L.tmp[1].cap;
}
static bool empty(const StubLane &L) {
    bool e = !L.pin.p && !L.pin.cap && !L.pin.ev[0] && !L.pin.ev[1] && !L.bf.p && !L.dscr.pw.p && !L.tmp[1].p;
    for (int i = 0; i < 4; ++i) e = e && !L.vp[i].p && !L.vp[i].cap;
    for (int i = 0; i < 24; ++i) e = e && !L.scr[i].p && !L.scr[i].cap;
    return e;
}
// mode 0: move construction, 1: move assignment onto a filled lane, 2: std::swap of two filled lanes, 3: a lane switch and back (cnmfe_lane::store / load)
static void run_lanestate(int mode) {
    int ok = 1, live_mid = -1;
    {
        StubLane a, b; fill(a, 1);
        const long long sa = sig(a); const void *pa = a.scr[2].p;
        if (mode == 0) { StubLane c(std::move(a)); ok = ok && empty(a) && sig(c) == sa && c.scr[2].p == pa; live_mid = g_live; }
        else if (mode == 1) { fill(b, 2); b = std::move(a); ok = ok && empty(a) && sig(b) == sa && b.scr[2].p == pa; live_mid = g_live; }
        else if (mode == 2) { fill(b, 2); const long long sb = sig(b); std::swap(a, b); ok = ok && sig(a) == sb && sig(b) == sa && b.scr[2].p == pa && a.kept.nnz == 7 && b.kept.nnz == 6; live_mid = g_live; }
        else { StubLane store0, store1; fill(store1, 2); const long long s1 = sig(store1);
               store0 = std::move(a); a = std::move(store1); store1.stream_ = nullptr;   // activate(1): the active state into lane 0's storage, lane 1's out of its own
               ok = ok && sig(a) == s1 && sig(store0) == sa && empty(store1) && !store1.stream_ && store0.scr[2].p == pa;
               store1 = std::move(a); a = std::move(store0); store0.stream_ = nullptr;   // activate(0)
               ok = ok && sig(a) == sa && sig(store1) == s1 && empty(store0) && !store0.stream_ && a.stream_ && a.scr[2].p == pa && a.kept.nnz == 6 && store1.kept.nnz == 7; live_mid = g_live; }
    }
    printf("%d %d %d\n", ok, live_mid, g_live);
}

int main(int argc, char **argv) {
    if (argc != 2) { fprintf(stderr, "usage: %s CASEFILE\n", argv[0]); return 2; }
    std::ifstream in(argv[1]);
    if (!in) { fprintf(stderr, "cannot read %s\n", argv[1]); return 2; }
    std::string line;
    while (std::getline(in, line)) {
        std::istringstream ss(line);
        std::string cmd; ss >> cmd;
        std::vector<long long> a; long long x;
        while (ss >> x) a.push_back(x);
        if ((cmd == "takes" || cmd == "legacy_takes") && a.size() == 16) printf("%d\n", cmd == "takes" ? run_takes(take_case(a)) : legacy_takes(take_case(a)));
        else if ((cmd == "serves" || cmd == "legacy_serves") && a.size() == 11) printf("%d\n", cmd == "serves" ? run_serves(serve_case(a)) : legacy_serves(serve_case(a)));
        else if (cmd == "kept" || cmd == "legacy_kept") run_kept(a, cmd == "legacy_kept");
        else if (cmd == "lanestate" && a.size() == 1) run_lanestate((int)a[0]);
        else { fprintf(stderr, "bad case: %s\n", line.c_str()); return 2; }
    }
    return 0;
}
