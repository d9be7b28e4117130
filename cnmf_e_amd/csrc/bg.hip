// B1/B2: ring-model background fit  ==  endoscope/fit_ring_model.m:1-127  on the resident block.
//
// The reference regresses, per patch pixel m, the centred background residual Bf(m,:) on the
// <=p ring neighbours Bf(ring(m),:) plus a constant: a (p+1)x(p+1) Gram + solve per pixel, with the
// operands GATHERED rows of one shared matrix (naive: 2*d*(p+1)^2*T flop and d*p*T gathered floats).
// MI355X formulation ("local covariance"):
//   B1  Bf = (Y - Ymean) - A*(C - Cmean)  written once, fp32, tiled as [16x16-pixel block][frame][256]
//   B2a Cov(a,b) = sum_t Bf(a,t)*Bf(b,t) for every pair of pixels whose 16x16 blocks are within
//       +-2 blocks: a block-sparse SYRK, 256x256xT' GEMMs on the fp64 MFMA pipe
//       (v_mfma_f64_16x16x4_f64; fp32 inputs are exact in fp64, accumulation is fp64 like MATLAB's)
//   B2b per pixel: gather the (p+1)^2 Gram and the RHS from the covariance table, add the ridge
//       1e-5*trace (fit_ring_model.m:106), Cholesky-solve in fp64 in LDS, write the p weights.
// Every ring pair of every patch pixel lies within +-2 blocks, so B2a computes each needed
// covariance exactly once (symmetric pairs once) instead of once per centre pixel.
#include "common.hpp"
#include "ring_solve_core.hpp"
#include "win_proj.hpp"
#include <type_traits>

namespace cnmfe {
// option win_i8_planes: 0 (default) = three digit planes of the video in the window projection when the sums run over at least 2048 frames (the rounding of a sample to
// 2^-23 of its pixel's largest value averages out with the number of frames: W 5e-7 .. 9e-7 of the oracle's at T = 3000 .. 20000), four for shorter recordings (T = 96:
// A moved by 2.2e-6, above the tests' 2e-6 -- and a short recording's projection costs microseconds either way); 3 / 4 force the choice
static inline bool win_planes3(cnmfe_ctx *ctx, int64_t T16) {
    const int64_t o = ctx->opt("win_i8_planes", 0);
    return o == 3 || (o != 4 && T16 * 16 >= 2048);
}


typedef float float4_t __attribute__((ext_vector_type(4)));

// ---- B1 ------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) k_build_bf(const float4 *__restrict__ Y4, int64_t Tc, BgGeom g,
                                                  const int *__restrict__ arow, const int *__restrict__ acol, const float *__restrict__ aval,
                                                  const float *__restrict__ Cc, int64_t ldc, float *__restrict__ bf, int tchunk, double *__restrict__ rs) {
    const int blk = blockIdx.x;                    // 16x16 block id, column-major over (nbr, nbc)
    const int bi = blk % g.nbr, bj = blk / g.nbr;
    const int lp = threadIdx.x;                    // local pixel in 4x4-patch order (lp_of)
    const int lr = ((lp >> 4) & 3) * 4 + (lp & 3), lc = (lp >> 6) * 4 + ((lp >> 2) & 3);
    const int rb = bi * BLK + lr, cb = bj * BLK + lc;
    const bool in = rb < g.nr_b && cb < g.nc_b;
    const int64_t q = in ? (int64_t)cb * g.nr_b + rb : 0;
    int e0 = 0, e1 = 0;
    if (in && arow) { e0 = arow[q]; e1 = arow[q + 1]; }
    const int64_t tp0 = (int64_t)blockIdx.y * tchunk;          // tchunk is a multiple of 4
    const int64_t tp1 = tp0 + tchunk < g.Tpad ? tp0 + tchunk : g.Tpad;
    float *out = bf + ((int64_t)blk * g.Tpad) * BLKPX + lp;
    if (g.kstride == 1) {                          // the video is resident centred: Bf = Yc - A*(C - Cmean), 4 frames per load
        for (int64_t tp = tp0; tp < tp1; tp += 4) {
            float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
            const int64_t c = tp >> 2;
            if (in && c < Tc) {
                v = Y4[c * g.d_b + q];
                for (int e = e0; e < e1; ++e) {
                    const float av = aval[e];
                    const float4 c4 = *reinterpret_cast<const float4 *>(Cc + (int64_t)acol[e] * ldc + tp);
                    v.x -= av * c4.x; v.y -= av * c4.y; v.z -= av * c4.z; v.w -= av * c4.w;
                }
            }
            if (g.bf4) reinterpret_cast<float4 *>(bf)[((int64_t)blk * (g.Tpad >> 2) + c) * BLKPX + lp] = v;
            else { out[tp * BLKPX] = v.x; out[(tp + 1) * BLKPX] = v.y; out[(tp + 2) * BLKPX] = v.z; out[(tp + 3) * BLKPX] = v.w; }
        }
    } else {                                       // frame subsampling Bf(:, 1:k:end)  (fit_ring_model.m:87)
        const float *Ys = reinterpret_cast<const float *>(Y4);
        for (int64_t tp = tp0; tp < tp1; ++tp) {
            float v = 0.f;
            if (in && tp < g.Tp) {
                const int64_t t = tp * g.kstride;
                v = Ys[((t >> 2) * g.d_b + q) * 4 + (t & 3)];
                for (int e = e0; e < e1; ++e) v -= aval[e] * Cc[(int64_t)acol[e] * ldc + t];
            }
            if (g.bf4) bf[(((int64_t)blk * (g.Tpad >> 2) + (tp >> 2)) * BLKPX + lp) * 4 + (tp & 3)] = v;
            else out[tp * BLKPX] = v;
        }
    }
}

// row sums of Bf over the used frames (the "ones" row of X, fit_ring_model.m:101)
__global__ void __launch_bounds__(256) k_rowsum(const float *__restrict__ bf, int64_t Tpad, double *__restrict__ rs, int bf4) {
    const int64_t blk = blockIdx.x;
    if (bf4) {
        const float4 *src4 = reinterpret_cast<const float4 *>(bf) + blk * (Tpad >> 2) * BLKPX + threadIdx.x;
        double s0 = 0, s1 = 0;
        for (int64_t c = 0; c < (Tpad >> 2); ++c) { const float4 v = src4[c * BLKPX]; s0 += (double)v.x + (double)v.z; s1 += (double)v.y + (double)v.w; }
        rs[blk * BLKPX + threadIdx.x] = s0 + s1;
        return;
    }
    const float *src = bf + blk * Tpad * BLKPX + threadIdx.x;
    double s0 = 0, s1 = 0;
    int64_t t = 0;
    for (; t + 1 < Tpad; t += 2) { s0 += src[t * BLKPX]; s1 += src[(t + 1) * BLKPX]; }
    if (t < Tpad) s0 += src[t * BLKPX];
    rs[blk * BLKPX + threadIdx.x] = s0 + s1;
}

// ---- B2a: block-sparse SYRK on the matrix pipe ------------------------------------------------------
// One workgroup = one 128x128 quadrant of one 256x256 block-pair covariance (16x16x4 MFMA: A[i=l&15][k=l>>4], B[k=l>>4][j=l&15]);
// K (= frames) advances GK = 16 per LDS stage.
constexpr int GK = 16;

// ---- dense tile slots ----------------------------------------------------------------------------------
// A first version gave every wave a FIXED 16-slot pattern of the quadrant with a `need` test per slot: hipcc turned that into two
// scalar branches per MFMA -- the issue stream, not the matrix pipe, was saturated (77 TF/s), and the four waves of a workgroup were
// unevenly loaded (84 %).  Here the host lists the needed 16x16 sub-tiles of
// every (displacement class, quadrant); tile t of an item goes to wave t%4, slot t/4, so slots are dense, the
// waves are balanced to within one tile, and the stage body is straight-line code instantiated per slot count.
// Bf is stored [block][frame/4][256][4] (like the resident video): a lane's A (or B) fragment for ALL FOUR
// k-steps of a 16-frame stage is ONE conflict-free ds_read_b128 (lane (l&15, l>>4) reads quad-row l>>4: MFMA m
// contracts frames {4*(l>>4) + m}), at lane base + a per-slot scalar tile offset.
constexpr int G4_NBUF = 4, G4_STAGE_F = 2 * GK * 128;

struct G4Wave {                       // per-wave constants of a work item (all wave-uniform except lbase, vo0, vo1)
    const float *gA, *gB;
    unsigned vo0, vo1, dA0;
    int lbase, nst, probe, ns, lane;
    double *out;                      // cov + pair*256*256 + (ih*128)*256 + jh*128
};

// the whole stage loop for a wave that owns NS slots (the last one only if `ns == NS`): instantiated per NS and
// selected ONCE per workgroup, so the loop body is branch-free straight-line code with its own register allocation
// (a switch inside the loop made hipcc keep the accumulators in scratch: 456 spilled VGPRs).
// fp64 MFMAs: exact products of the fp32 operands, fp64 sums.  Rounds 1-4 also carried an fp32-MFMA mode with fp64 shadow accumulation (89 ms at H, W error 2e-4)
// and a split-bf16 mode (4 bf16 products per fp32 product, 50 ms, 9e-5) for the direct Gram: both retired in round 5, when the int8 digit Gram (gram_i8.hpp: 64 ms,
// EXACT up to a 32-bit quantisation, 1e-8 of W) took over every use that fits its int32 range -- this kernel remains for the outlier branch (a clipped, frame-selected
// Bf) and for recordings beyond 24576 used frames.
template <int NS>
__device__ __forceinline__ void gram4_run(const G4Wave &w, const float *smem, const int *__restrict__ tlw) {
    int ao[NS], bo[NS], ti[NS], tj[NS];
#pragma unroll
    for (int sl = 0; sl < NS; ++sl) {
        const int code = __builtin_amdgcn_readfirstlane(sl < w.ns ? tlw[sl * 4] : 0);
        ti[sl] = code & 7; tj[sl] = code >> 4;
        ao[sl] = ti[sl] * 64; bo[sl] = GK * 128 + tj[sl] * 64;
    }
    const bool last = w.ns == NS;
    auto issue = [&](int st) {
        int sc = st < w.nst ? st : w.nst - 1;                            // clamp: keeps the vmcnt arithmetic uniform
        if (w.probe & 1) sc = 0;                                         // A/B probe (gram_probe bit 0): every stage re-reads stage 0 -> no fabric traffic
        const float *sa = w.gA + (int64_t)sc * GK * BLKPX, *sb = w.gB + (int64_t)sc * GK * BLKPX;
        const unsigned d = w.dA0 + (unsigned)(st & (G4_NBUF - 1)) * (G4_STAGE_F * 4u);
        glds16(sa, w.vo0, d); glds16(sa, w.vo1, d + 4096u);
        glds16(sb, w.vo0, d + 8192u); glds16(sb, w.vo1, d + 12288u);
    };
    double4_t acc[NS];
#pragma unroll
    for (int sl = 0; sl < NS; ++sl) acc[sl] = (double4_t){0.0, 0.0, 0.0, 0.0};
#pragma unroll
    for (int s0 = 0; s0 < G4_NBUF - 1; ++s0) issue(s0);
    for (int st = 0; st < w.nst; ++st) {
        if (!(w.probe & 2)) {                                                         // (gram_probe bit 1: timing experiment without the stage sync)
        asm volatile("s_waitcnt vmcnt(%0)" :: "i"(4 * (G4_NBUF - 2)) : "memory");    // this wave's part of stage st has landed
        __builtin_amdgcn_s_barrier();                                                // ... and everybody else's; buffer st-1 is free
        }
        asm volatile("" ::: "memory");
        issue(st + G4_NBUF - 1);
        int lb = w.lbase;
        asm volatile("" : "+v"(lb));            // opaque per stage: no hoisting of 2*NS per-slot address VGPRs out of the loop
        const float *lp = smem + (st & (G4_NBUF - 1)) * G4_STAGE_F + lb;
        // slots go in batches of two: the fragments of the next batch (4 ds_read_b128) are issued before the current
        // batch's MFMAs, and the two slots' MFMA chains are interleaved so that no MFMA waits on its predecessor's
        // result (the one-slot version stalled an LDS latency per slot: hipcc waited lgkmcnt(0) before every chain)
        float4 fa[2][2], fb[2][2];
        auto ldb = [&](int buf, int base) {
#pragma unroll
            for (int u = 0; u < 2; ++u)
                if (base + u < NS) {
                    fa[buf][u] = *reinterpret_cast<const float4 *>(lp + ao[base + u]);
                    fb[buf][u] = *reinterpret_cast<const float4 *>(lp + bo[base + u]);
                }
        };
        ldb(0, 0);
#pragma unroll
        for (int base = 0; base < NS; base += 2) {
            const int cur = (base >> 1) & 1;
            if (base + 2 < NS) ldb(cur ^ 1, base + 2);
            asm volatile("" ::: "memory");
            const bool on0 = true, on1 = (base + 1 < NS - 1) || (base + 1 == NS - 1 && last);
            const bool only0_last = (base == NS - 1);                   // odd NS: the last slot stands alone
            const bool do0 = only0_last ? last : on0;
#pragma unroll
            for (int kq = 0; kq < 4; ++kq) {
#pragma unroll
                for (int u = 0; u < 2; ++u) {
                    if (base + u >= NS) continue;
                    if (u == 0 ? !do0 : !on1) continue;
                    const float av = kq == 0 ? fa[cur][u].x : kq == 1 ? fa[cur][u].y : kq == 2 ? fa[cur][u].z : fa[cur][u].w;
                    const float bv = kq == 0 ? fb[cur][u].x : kq == 1 ? fb[cur][u].y : kq == 2 ? fb[cur][u].z : fb[cur][u].w;
                    acc[base + u] = __builtin_amdgcn_mfma_f64_16x16x4f64((double)av, (double)bv, acc[base + u], 0, 0, 0);
                }
            }
        }
        asm volatile("" ::: "memory");
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");                  // drain the clamped tail loads before the LDS is released
    const int fl = w.lane & 15;
#pragma unroll
    for (int sl = 0; sl < NS; ++sl)
        if (sl < NS - 1 || last) {
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int rr = (w.lane >> 4) + 4 * r;                    // D layout (fp64 16x16): row = (lane >> 4) + 4 r
                w.out[(int64_t)(ti[sl] * 16 + rr) * BLKPX + tj[sl] * 16 + fl] = acc[sl][r];
            }
        }
}

__global__ void __launch_bounds__(256, 2) k_gram4(const float *__restrict__ bf, int64_t Tpad, const int4 *__restrict__ pairs,
                                                  const int *__restrict__ work, int nwork, const int *__restrict__ tl_cnt,
                                                  const int *__restrict__ tl, int probe, double *__restrict__ cov) {
    extern __shared__ __attribute__((aligned(16))) float smem[];       // the ONLY LDS object (a second one de-pipelines the DMA)
    const int nwg = gridDim.x;
    int bid = blockIdx.x;
    if (nwg % 8 == 0) bid = (blockIdx.x % 8) * (nwg / 8) + blockIdx.x / 8;
    if (bid >= nwork) return;
    const int wk = work[bid];
    const int pair = wk >> 2, quad = wk & 3;
    const int ih = quad & 1, jh = quad >> 1;
    const int4 pr = pairs[pair];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int lidx = pr.z * 4 + quad;
    const int cnt = __builtin_amdgcn_readfirstlane(tl_cnt[lidx]);
    G4Wave w;
    w.gA = bf + ((int64_t)pr.x * Tpad) * BLKPX + ih * 512;             // a quad-row is 256 px x 4 frames; half ih starts at px 128
    w.gB = bf + ((int64_t)pr.y * Tpad) * BLKPX + jh * 512;
    // DMA: one wave-instruction = 64 px x 4 frames (1 KB) of one quad-row.  Per half and stage: 4 quad-rows x 2 = 8
    // instructions; wave w moves instruction w (quad-row w>>1, pixels (w&1)*64..) and w+4 (quad-row 2 + (w>>1)).
    w.vo0 = (unsigned)((((wave >> 1) * BLKPX + (wave & 1) * 64 + lane) * 4) * 4);
    w.vo1 = w.vo0 + 2u * BLKPX * 4u * 4u;
    w.dA0 = (unsigned)(uintptr_t)(__attribute__((address_space(3))) float *)smem + (unsigned)wave * 1024u;
    w.lbase = (lane >> 4) * 512 + (lane & 15) * 4;                     // quad-row l>>4, pixel l&15 of the tile, 4 frames
    w.nst = (int)(Tpad / GK); w.probe = probe; w.lane = lane;
    w.ns = cnt > wave ? (cnt - wave + 3) >> 2 : 0;                     // tiles wave, wave+4, ...
    w.out = cov + (int64_t)pair * BLKPX * BLKPX + (int64_t)(ih * 128) * BLKPX + jh * 128;
    const int *tlw = tl + lidx * 64 + wave;
    switch ((cnt + 3) >> 2) {                                          // slots of the busiest wave; the others skip the last one
#define G4_CASE(N) case N: gram4_run<N>(w, smem, tlw); break;
        G4_CASE(1) G4_CASE(2) G4_CASE(3) G4_CASE(4) G4_CASE(5) G4_CASE(6) G4_CASE(7) G4_CASE(8)
        G4_CASE(9) G4_CASE(10) G4_CASE(11) G4_CASE(12) G4_CASE(13) G4_CASE(14) G4_CASE(15) G4_CASE(16)
#undef G4_CASE
        default: break;
    }
}

// ---- B2a', incremental: Cov(Bf) from the covariance of the VIDEO ------------------------------------------------
// Bf = Yc - A Cc (fit_ring_model.m:45-47), so  sum_t Bf_i Bf_j = sum_t Yc_i Yc_j - sum_k A_jk U~_ik - sum_k A_ik U~_jk  with
// U~_ik = sum_t (Yc_i - 1/2 sum_l A_il Cc_l)(t) Cc_k(t)   (the 1/2 shares the A G A' term between the two sums; G = Cc Cc').
// The first term does not depend on A, C: it is computed ONCE per patch and frame stride on the fp64 matrix pipe (the block-sparse
// SYRK above on Yc alone) and kept; every later fit only needs U~ for pixels within two 16x16 blocks of a footprint -- per block a
// (256 px) x (footprints near it, <= 64) x T' GEMM on the fp64 pipe, 0.1-0.2 TFLOP instead of 9.6 -- and one sweep over the table.
// Everything is fp64 (exact fp32 products, fp64 sums): the difference of the two large terms keeps ~1e-13 relative accuracy.
// csum[k] = sum over the used frames of Cc_k  (the ones-row of X: rowsum(Bf) = rowsum(Yc) - A csum)
__global__ void __launch_bounds__(256) k_trace_subsum(const float *__restrict__ Cc, int64_t ldc, int64_t Tp, int kstride, double *__restrict__ csum) {
    const float *row = Cc + (int64_t)blockIdx.x * ldc;
    __shared__ double red[256];
    double s = 0;
    for (int64_t tp = threadIdx.x; tp < Tp; tp += 256) s += (double)row[tp * kstride];
    red[threadIdx.x] = s; __syncthreads();
    for (int o = 128; o > 0; o >>= 1) { if ((int)threadIdx.x < o) red[threadIdx.x] += red[threadIdx.x + o]; __syncthreads(); }
    if (threadIdx.x == 0) csum[blockIdx.x] = red[0];
}

// U(i,k) = sum_t Yc_i(t) Cc_k(t) for the 256 pixels of a block and the (<= 16 NT) traces on its list, plus G(k,l) = sum_t Cc_k Cc_l on the same
// list: plain GEMMs on the fp64 matrix pipe with both operands read straight from global memory -- lane (fi, kq) of a 16x16x4 fragment wants
// ONE float (pixel fi of a 4x4 patch / trace fi of a 16-trace group, frame kq of the chunk), and the 64 lanes of a pixel fragment cover four
// full 64-byte segments of the 4-frame-interleaved video.  No LDS, no barriers; loads run two chunks ahead of the MFMAs.  One launch covers
// all blocks (longest lists first) x frame segments; partial sums go to per-segment buffers that k_win_fix adds in a fixed order.
// (A first version staged Z = Yc - 1/2 A Cc through LDS with two barriers per chunk and one launch per list length: 7.5 ms.)
template <int NT>
__device__ __forceinline__ void win_body(const float4 *__restrict__ Y4, const BgGeom &g, const float *__restrict__ Cc, int64_t ldc, int blk, int l0, int nl,
                                         const int *__restrict__ lst_k, int64_t c0, int64_t c1, double *__restrict__ Ut, double *__restrict__ Gb) {
    const int bi = blk % g.nbr, bj = blk / g.nbr;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, fi = lane & 15, kq = lane >> 4;
    const float *Ys = reinterpret_cast<const float *>(Y4);
    const float *ya[4]; const float *tb[NT];
#pragma unroll
    for (int a = 0; a < 4; ++a) {
        const int lp = (wave * 4 + a) * 16 + fi;
        const int lr = ((lp >> 4) & 3) * 4 + (lp & 3), lc = (lp >> 6) * 4 + ((lp >> 2) & 3);
        const int rb = bi * BLK + lr, cb = bj * BLK + lc;
        ya[a] = (rb < g.nr_b && cb < g.nc_b) ? Ys + ((int64_t)cb * g.nr_b + rb) * 4 : nullptr;
    }
#pragma unroll
    for (int b = 0; b < NT; ++b) { const int sl = b * 16 + fi; tb[b] = sl < nl ? Cc + (int64_t)lst_k[l0 + sl] * ldc : nullptr; }
    double4_t acc[4][NT], accg[NT];
#pragma unroll
    for (int b = 0; b < NT; ++b) {
        accg[b] = (double4_t){0.0, 0.0, 0.0, 0.0};
#pragma unroll
        for (int a = 0; a < 4; ++a) acc[a][b] = (double4_t){0.0, 0.0, 0.0, 0.0};
    }
    struct Frag { float y[4]; float t[NT]; };
    auto load = [&](int64_t c) {
        Frag f;
        const int64_t tp = 4 * c + kq, t = tp * g.kstride;
        const bool on = c < c1 && tp < g.Tp;
        const int64_t yo = ((t >> 2) * g.d_b) * 4 + (t & 3);
#pragma unroll
        for (int a = 0; a < 4; ++a) f.y[a] = (on && ya[a]) ? ya[a][yo] : 0.f;
#pragma unroll
        for (int b = 0; b < NT; ++b) f.t[b] = (on && tb[b]) ? tb[b][t] : 0.f;
        return f;
    };
    const bool gw = wave < NT;                              // wave w also owns row-group w of G
    auto mm = [&](const Frag &f) {
        double bv[NT];
#pragma unroll
        for (int b = 0; b < NT; ++b) bv[b] = (double)f.t[b];
#pragma unroll
        for (int a = 0; a < 4; ++a) {
            const double av = (double)f.y[a];
#pragma unroll
            for (int b = 0; b < NT; ++b) acc[a][b] = __builtin_amdgcn_mfma_f64_16x16x4f64(av, bv[b], acc[a][b], 0, 0, 0);
        }
        if (gw) {
            double gv = bv[0];
#pragma unroll
            for (int b = 1; b < NT; ++b) gv = wave == b ? bv[b] : gv;
#pragma unroll
            for (int b = 0; b < NT; ++b) accg[b] = __builtin_amdgcn_mfma_f64_16x16x4f64(gv, bv[b], accg[b], 0, 0, 0);
        }
    };
    // loads run WIN_AHEAD chunks in front of the MFMAs; loads past the segment return zeros.  (Measured at H: 2 ahead 5.5 ms, 3 ahead 5.4 ms,
    // 6 ahead 6.0 ms -- each extra chunk costs 18 VGPRs and beyond 256 the kernel drops to one wave per SIMD; with lists of ~48 traces the
    // 13 fp64 MFMAs per chunk and wave are ~4 ms of matrix-pipe time at the clock this kernel runs at, so latency is not what is left.)
    Frag f[WIN_AHEAD];
#pragma unroll
    for (int d = 0; d < WIN_AHEAD; ++d) f[d] = load(c0 + d);
    for (int64_t c = c0; c < c1; c += WIN_AHEAD) {
#pragma unroll
        for (int d = 0; d < WIN_AHEAD; ++d) {
            const Frag nx = load(c + WIN_AHEAD + d);
            mm(f[d]);
            f[d] = nx;
        }
    }
    // D layout (fp64 16x16): row = (lane>>4) + 4r, col = lane&15
#pragma unroll
    for (int b = 0; b < NT; ++b) {
        const int slot = b * 16 + fi;
#pragma unroll
        for (int a = 0; a < 4; ++a)
            if (slot < nl)
#pragma unroll
                for (int r = 0; r < 4; ++r) Ut[(int64_t)(l0 + slot) * BLKPX + (wave * 4 + a) * 16 + kq + 4 * r] = acc[a][b][r];
        if (gw)
#pragma unroll
            for (int r = 0; r < 4; ++r) Gb[(int64_t)blk * WIN_NLB * WIN_NLB + (wave * 16 + kq + 4 * r) * WIN_NLB + slot] = accg[b][r];
    }
}

__global__ void __launch_bounds__(256) k_win_proj(const float4 *__restrict__ Y4, BgGeom g, const float *__restrict__ Cc, int64_t ldc, const int *__restrict__ lst_ptr,
                                                  const int *__restrict__ lst_k, const int *__restrict__ blk_list, int nseg, double *__restrict__ Ut, int64_t ut_stride,
                                                  double *__restrict__ Gb, int64_t gb_stride) {
    const int blk = blk_list[blockIdx.x / nseg], seg = blockIdx.x % nseg;
    const int l0 = lst_ptr[blk], nl = lst_ptr[blk + 1] - l0;
    double *ut = Ut + seg * ut_stride, *gb = Gb + seg * gb_stride;
    const int64_t nchunk = (g.Tp + 3) >> 2;
    int64_t cseg = ((nchunk + nseg - 1) / nseg + 1) & ~int64_t(1);
    const int64_t c0 = seg * cseg, c1 = c0 + cseg < nchunk ? c0 + cseg : nchunk;
    switch ((nl + 15) >> 4) {
        case 1: win_body<1>(Y4, g, Cc, ldc, blk, l0, nl, lst_k, c0, c1, ut, gb); break;
        case 2: win_body<2>(Y4, g, Cc, ldc, blk, l0, nl, lst_k, c0, c1, ut, gb); break;
        case 3: win_body<3>(Y4, g, Cc, ldc, blk, l0, nl, lst_k, c0, c1, ut, gb); break;
        case 4: win_body<4>(Y4, g, Cc, ldc, blk, l0, nl, lst_k, c0, c1, ut, gb); break;
        default: break;
    }
}

// U~(i,k) = sum_seg U_seg(i,k) - 1/2 sum_{l at i} A_il sum_seg G_seg(l,k), written to segment 0.
// Workgroup = (block, WF_S traces of its list): a small patch has ~100 blocks but 16 frame segments, and one workgroup per block summed its
// 16 x (list length + 16) strided partials in one serial loop per thread -- 0.21 ms per launch against 0.06 ms for the whole 512 x 512 frame.
constexpr int WF_S = 4;
__global__ void __launch_bounds__(256) k_win_fix(BgGeom g, int K, const int *__restrict__ arow, const int *__restrict__ acol, const float *__restrict__ aval,
                                                 const int *__restrict__ lst_ptr, const short *__restrict__ slot_of, const int *__restrict__ blk_list, int nseg,
                                                 double *__restrict__ Ut, int64_t ut_stride, const double *__restrict__ Gb, int64_t gb_stride, double *__restrict__ Praw,
                                                 const double *__restrict__ GK, const int *__restrict__ lst_k) {
    __shared__ double G[WIN_NLB * WF_S];                     // G[r][j]: column s0 + j of the block's list Gram matrix
    const int blk = blk_list[blockIdx.x];
    const int l0 = lst_ptr[blk], nl = lst_ptr[blk + 1] - l0;
    const int s0 = (int)blockIdx.y * WF_S;
    if (s0 >= nl) return;
    const int lp = threadIdx.x;
    const int nlp = ((nl + 15) >> 4) << 4;
    {
        const int r = lp / WF_S, c = s0 + lp % WF_S;         // WIN_NLB * WF_S == 256: one entry per thread
        double v = 0.0;
        if (GK) {                                            // (win_proj_i8.hpp: one K x K Gram matrix of the centred traces per fit instead of per-block, per-segment copies)
            if (r < nl && c < nl) v = GK[(int64_t)lst_k[l0 + r] * K + lst_k[l0 + c]];
        } else if (r < nlp && c < nlp) {
            const double *gp = Gb + (int64_t)blk * WIN_NLB * WIN_NLB + r * WIN_NLB + c;
#pragma unroll 4
            for (int sg = 0; sg < nseg; ++sg) v += gp[sg * gb_stride];
        }
        G[lp] = v;
    }
    __syncthreads();
    const int lr = ((lp >> 4) & 3) * 4 + (lp & 3), lc = (lp >> 6) * 4 + ((lp >> 2) & 3);
    const int rb = (blk % g.nbr) * BLK + lr, cb = (blk / g.nbr) * BLK + lc;
    int e0 = 0, e1 = 0;
    if (rb < g.nr_b && cb < g.nc_b) { const int64_t q = (int64_t)cb * g.nr_b + rb; e0 = arow[q]; e1 = arow[q + 1]; }
    const int s1 = s0 + WF_S < nl ? s0 + WF_S : nl;
    for (int s = s0; s < s1; ++s) {
        double *u = Ut + (int64_t)(l0 + s) * BLKPX + lp;
        double v = u[0];
#pragma unroll 4
        for (int sg = 1; sg < nseg; ++sg) v += u[sg * ut_stride];
        double w = 0.0;
        for (int e = e0; e < e1; ++e) w += (double)aval[e] * G[(int)slot_of[(int64_t)blk * K + acol[e]] * WF_S + (s - s0)];
        u[0] = v - 0.5 * w;
        if (Praw) Praw[(int64_t)(l0 + s) * BLKPX + lp] = v;      // U itself = Yc Cc' on the block: the P table of the sweep-free spatial update (vproj.hip)
    }
}
static_assert(WIN_NLB * WF_S == 256, "k_win_fix: one Gram entry per thread");

// cov(pair)(i,j) = base(pair)(i,j) - sum_{k at j} A_jk U~_a(k, i) - sum_{k at i} A_ik U~_b(k, j)  over the needed 16x16 sub-tiles
// Thread = (half h, row ty of a sub-tile, column PAIR tx2): 16-byte loads and stores (one wave instruction moves 1 KB of the 7.7 GB sweep); the two
// 128-thread halves of the workgroup take the row patches pi, pi + 1 side by side (a half is two whole waves: their need masks may differ).
__global__ void __launch_bounds__(256) k_cov_correct(const double *__restrict__ base, double *__restrict__ cov, const int4 *__restrict__ pairs,
                                                     const unsigned short *__restrict__ needmask, BgGeom g, int K, const int *__restrict__ arow,
                                                     const int *__restrict__ acol, const float *__restrict__ aval, const int *__restrict__ lst_ptr,
                                                     const short *__restrict__ slot_of, const double *__restrict__ Ut) {
    const int pair = blockIdx.x;
    const int4 pr = pairs[pair];
    const int ba = pr.x, bb = pr.y, rel = pr.z;
    const int half = threadIdx.x >> 7, ty = (threadIdx.x >> 3) & 15, tx = (threadIdx.x & 7) * 2;
    const int la = lst_ptr[ba], lb = lst_ptr[bb];
    auto pix = [&](int blk, int lp, int &e0, int &e1) {
        const int lr = ((lp >> 4) & 3) * 4 + (lp & 3), lc = (lp >> 6) * 4 + ((lp >> 2) & 3);
        const int rb = (blk % g.nbr) * BLK + lr, cb = (blk / g.nbr) * BLK + lc;
        e0 = e1 = 0;
        if (rb < g.nr_b && cb < g.nc_b) { const int64_t q = (int64_t)cb * g.nr_b + rb; e0 = arow[q]; e1 = arow[q + 1]; }
    };
    const double *bp = base + (int64_t)pair * BLKPX * BLKPX;
    double *cp = cov + (int64_t)pair * BLKPX * BLKPX;
    // gridDim.y workgroups share a pair (its 16 row patches split evenly): a small patch has too few pairs to fill the chip with one each
    const int pi0 = (int)blockIdx.y * (16 / (int)gridDim.y), pi1 = pi0 + 16 / (int)gridDim.y;
    for (int pi = pi0 + half; pi < pi1; pi += 2) {
        const unsigned mask = needmask[rel * 16 + pi];
        if (!mask) continue;
        const int ilp = pi * 16 + ty;
        int ei0, ei1; pix(ba, ilp, ei0, ei1);
        for (int pj = 0; pj < 16; ++pj) {
            if (!((mask >> pj) & 1u)) continue;
            const int jlp = pj * 16 + tx;
            int ej0, ej1, ek0, ek1; pix(bb, jlp, ej0, ej1); pix(bb, jlp + 1, ek0, ek1);
            const int idx = ilp * BLKPX + jlp;
            double2 v = *reinterpret_cast<const double2 *>(bp + idx);
            for (int e = ej0; e < ej1; ++e) v.x -= (double)aval[e] * Ut[(int64_t)(la + slot_of[(int64_t)ba * K + acol[e]]) * BLKPX + ilp];
            for (int e = ek0; e < ek1; ++e) v.y -= (double)aval[e] * Ut[(int64_t)(la + slot_of[(int64_t)ba * K + acol[e]]) * BLKPX + ilp];
            for (int e = ei0; e < ei1; ++e) {
                const double2 u = *reinterpret_cast<const double2 *>(Ut + (int64_t)(lb + slot_of[(int64_t)bb * K + acol[e]]) * BLKPX + jlp);
                v.x -= (double)aval[e] * u.x; v.y -= (double)aval[e] * u.y;
            }
            *reinterpret_cast<double2 *>(cp + idx) = v;
        }
    }
}

__global__ void __launch_bounds__(256) k_rowsum_correct(const double *__restrict__ base, double *__restrict__ rs, BgGeom g, const int *__restrict__ arow,
                                                        const int *__restrict__ acol, const float *__restrict__ aval, const double *__restrict__ csum) {
    const int blk = blockIdx.x, lp = threadIdx.x;
    const int lr = ((lp >> 4) & 3) * 4 + (lp & 3), lc = (lp >> 6) * 4 + ((lp >> 2) & 3);
    const int rb = (blk % g.nbr) * BLK + lr, cb = (blk / g.nbr) * BLK + lc;
    double v = base[(int64_t)blk * BLKPX + lp];
    if (rb < g.nr_b && cb < g.nc_b) {
        const int64_t q = (int64_t)cb * g.nr_b + rb;
        for (int e = arow[q]; e < arow[q + 1]; ++e) v -= (double)aval[e] * csum[acol[e]];
    }
    rs[(int64_t)blk * BLKPX + lp] = v;
}

// ---- helpers on the covariance table ----------------------------------------------------------------
struct CovTab {
    const double *cov; const int *pair_of;   // pair_of[blk*nrel + rel] or -1
    const int *wcodes; int woff;             // [(bc0 + woff) * (nbr + 2 woff) + (br0 + woff)][256]: the block-pair codes of the 4 x 4-block window with origin (br0, bc0) >= -woff, k_win_codes
    int nbr, nbc;
    int maxd, nrel;                          // largest block displacement between two ring pixels of one centre (2: radius <= 16, 3: <= 24); nrel_of(maxd)
};

// The block-pair codes of a pixel's 4 x 4-block window depend on the window's origin only, so they are tabulated once per fit instead of being
// re-derived (25 integer operations and a dependent load per entry, 256 entries) by every pixel's wave.
__global__ void __launch_bounds__(256) k_win_codes(const int *__restrict__ pair_of, int nbr, int nbc, int woff, int maxd, int nrel, int *__restrict__ wcodes) {
    const int br0 = (int)(blockIdx.x % (nbr + 2 * woff)) - woff, bc0 = (int)(blockIdx.x / (nbr + 2 * woff)) - woff;
    const int q = threadIdx.x, a = q >> 4, b = q & 15;
    int ia = br0 + (a & 3), ja = bc0 + (a >> 2), ib = br0 + (b & 3), jb = bc0 + (b >> 2);
    int code = -1;
    if (ia >= 0 && ja >= 0 && ib >= 0 && jb >= 0 && ia < nbr && ib < nbr && ja < nbc && jb < nbc) {
        int dR = ib - ia, dC = jb - ja, sw = 0;
        if (dC < 0 || (dC == 0 && dR < 0)) { sw = 1; ia = ib; ja = jb; dR = -dR; dC = -dC; }
        if (dC <= maxd && dR <= maxd && dR >= -maxd) {
            const int pidx = pair_of[(ja * nbr + ia) * nrel + rel_index(dR, dC, maxd)];
            code = pidx < 0 ? -1 : ((pidx << 2) | (sw << 1) | ((dR == 0 && dC == 0) ? 1 : 0));
        }
    }
    wcodes[(int64_t)blockIdx.x * 256 + q] = code;
}
}  // namespace cnmfe
#include "ring_solve.hpp"
#include "ring_solve_packed.hpp"
#include "ring_solve_inv.hpp"
#include "ring_solve_staged.hpp"
#include "gram_i8.hpp"
#include "win_proj_i8.hpp"
namespace cnmfe {

// sum(A, 2) of the block region out of the CSR rows the fit uploads anyway: per row the fp64 sum of its entries in the order they are stored, rounded to fp32 once
// (what the host loop did before its result went over the bus); arow == nullptr: the constant `fillv` (A = ones(d, 1), or no entries at all)
__global__ void __launch_bounds__(256) k_asum(const int *__restrict__ arow, const float *__restrict__ aval, float fillv, int64_t n, float *__restrict__ asum) {
    const int64_t q = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (q >= n) return;
    if (!arow) { asum[q] = fillv; return; }
    double s = 0;
    for (int e = arow[q]; e < arow[q + 1]; ++e) s += aval[e];
    asum[q] = (float)s;
}
// slot_of[b * K + k] = position of neuron k in block b's list lst_k[lst_ptr[b] ..) -- the inverse of the lists that are on the device already; the caller has
// filled the table with -1.  One workgroup per block.
__global__ void __launch_bounds__(64) k_slot_build(const int *__restrict__ lst_ptr, const int *__restrict__ lst_k, int K, short *__restrict__ slot_of) {
    const int b = blockIdx.x, p0 = lst_ptr[b], n = lst_ptr[b + 1] - p0;
    for (int s = threadIdx.x; s < n; s += blockDim.x) slot_of[(int64_t)b * K + lst_k[p0 + s]] = (short)s;
}

// ind_active = abs(W_old)*sum(A,2) > 0  (fit_ring_model.m:28)
__global__ void k_active(const float *__restrict__ W, BgGeom g, const int *__restrict__ dr, const int *__restrict__ dc,
                         const float *__restrict__ asum, unsigned char *__restrict__ active, int *__restrict__ nactive) {
    int64_t m = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    int on = 0;
    if (m < g.d) {
        const int rbm = (int)(m % g.nr) + g.roff, cbm = (int)(m / g.nr) + g.coff;
        float s = 0.f;
        // eight offsets at a time, every load unconditional (neighbours outside the block read pixel 0 and are masked): the loads of a group are
        // independent, one load behind a branch per trip made the kernel 2 x 96 memory latencies long.  The sum keeps the ring order.
        for (int i0 = 0; i0 < g.p; i0 += 8) {
            float w8[8], a8[8];
#pragma unroll
            for (int u = 0; u < 8; ++u) {
                const int i = i0 + u < g.p ? i0 + u : g.p - 1;
                const int rb = rbm + dr[i], cb = cbm + dc[i];
                const bool in = i0 + u < g.p && rb >= 0 && rb < g.nr_b && cb >= 0 && cb < g.nc_b;
                w8[u] = W[(int64_t)i * g.d + m];
                a8[u] = asum[in ? (int64_t)cb * g.nr_b + rb : 0];
                if (!in) w8[u] = 0.f;
            }
#pragma unroll
            for (int u = 0; u < 8; ++u) if (w8[u] != 0.f) s += fabsf(w8[u]) * a8[u];
        }
        on = s > 0.f;
        active[m] = (unsigned char)on;
    }
    unsigned long long b = __ballot(on);
    if ((threadIdx.x & 63) == 0) atomicAdd(nactive, (int)__popcll(b));
}

// b0 = Ymean(ind_patch) - A(ind_patch,:)*Cmean   (fit_ring_model.m:44), double
__global__ void k_b0(const double *__restrict__ ymean, BgGeom g, const int *__restrict__ arow, const int *__restrict__ acol,
                     const float *__restrict__ aval, const double *__restrict__ Cmean, double *__restrict__ b0) {
    int64_t m = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (m >= g.d) return;
    const int64_t q = (int64_t)((int)(m / g.nr) + g.coff) * g.nr_b + (int)(m % g.nr) + g.roff;
    double v = ymean[q];
    if (arow) for (int e = arow[q]; e < arow[q + 1]; ++e) v -= (double)aval[e] * Cmean[acol[e]];
    b0[m] = v;
}

// ---- outlier branch (fit_ring_model.m:50-56): Bf_old = W_old*Bf; entries of the patch rows above Bf_old + thresh*sn take the value of
// Bf_old.  Bf_old is formed from the unmodified Bf (the reference computes it before touching tmp_Bf), so the clipped rows go to a
// second buffer.  One thread per (patch pixel, 4 frames); cnt[t] = sum(ind_outlier(:, t)) feeds the frame selection of :62-67.
__device__ __forceinline__ int64_t bf4_index(const BgGeom &g, int rb, int cb, int64_t c) {
    return ((int64_t)((cb >> 4) * g.nbr + (rb >> 4)) * (g.Tpad >> 2) + c) * BLKPX + lp_of(rb & 15, cb & 15);
}
__global__ void __launch_bounds__(256) k_outlier_clip(const float4 *__restrict__ bf, float4 *__restrict__ bf2, BgGeom g, const int *__restrict__ dr,
                                                      const int *__restrict__ dc, const float *__restrict__ W, const float *__restrict__ sn_b,
                                                      double thresh, int *__restrict__ cnt) {
    const int64_t m = (int64_t)blockIdx.x * blockDim.x + threadIdx.x, c = blockIdx.y;
    if (m >= g.d) return;
    const int rbm = (int)(m % g.nr) + g.roff, cbm = (int)(m / g.nr) + g.coff;
    double o0 = 0, o1 = 0, o2 = 0, o3 = 0;
    for (int i = 0; i < g.p; ++i) {
        const float w = W[(int64_t)i * g.d + m];
        if (w == 0.f) continue;                                   // outside the FOV (or an exact zero: no term either way)
        const float4 v = bf[bf4_index(g, rbm + dr[i], cbm + dc[i], c)];
        o0 += (double)w * v.x; o1 += (double)w * v.y; o2 += (double)w * v.z; o3 += (double)w * v.w;
    }
    const int64_t at = bf4_index(g, rbm, cbm, c);
    float4 y = bf[at];
    const double lim = thresh * (double)sn_b[(int64_t)cbm * g.nr_b + rbm];
    const int64_t t = c * 4;
    if (t < g.T && (double)y.x > o0 + lim) { y.x = (float)o0; atomicAdd(&cnt[t], 1); }
    if (t + 1 < g.T && (double)y.y > o1 + lim) { y.y = (float)o1; atomicAdd(&cnt[t + 1], 1); }
    if (t + 2 < g.T && (double)y.z > o2 + lim) { y.z = (float)o2; atomicAdd(&cnt[t + 2], 1); }
    if (t + 3 < g.T && (double)y.w > o3 + lim) { y.w = (float)o3; atomicAdd(&cnt[t + 3], 1); }
    bf2[at] = y;
}
// Bf = Bf(:, ind_frames) (:66): frame j of the destination is frame sel[j] of the source; frames past nsel are zero padding
__global__ void __launch_bounds__(256) k_select_frames(const float *__restrict__ src, int64_t Tpad_src, float *__restrict__ dst, int64_t Tpad_dst,
                                                       const int *__restrict__ sel, int64_t nsel) {
    const int64_t blk = blockIdx.x, lp = threadIdx.x;
    for (int64_t c = blockIdx.y; c < (Tpad_dst >> 2); c += gridDim.y) {
        float v[4];
        for (int i = 0; i < 4; ++i) {
            const int64_t j = c * 4 + i;
            float x = 0.f;
            if (j < nsel) { const int64_t t = sel[j]; x = src[((blk * (Tpad_src >> 2) + (t >> 2)) * BLKPX + lp) * 4 + (t & 3)]; }
            v[i] = x;
        }
        reinterpret_cast<float4 *>(dst)[(blk * (Tpad_dst >> 2) + c) * BLKPX + lp] = make_float4(v[0], v[1], v[2], v[3]);
    }
}
// quantile(x, q) of the Statistics Toolbox as documented: the sorted values are the (0.5/n), (1.5/n), ... quantiles, linear
// interpolation between them, the extremes outside
static double matlab_quantile(std::vector<int> x, double q) {
    std::sort(x.begin(), x.end());
    const int64_t n = (int64_t)x.size();
    const double r = q * (double)n + 0.5;                 // 1-based fractional rank
    if (r <= 1.0) return x[0];
    if (r >= (double)n) return x[n - 1];
    const int64_t lo = (int64_t)std::floor(r);
    return x[lo - 1] + (r - (double)lo) * (double)(x[lo] - x[lo - 1]);
}

// ---- one NT dispatch: f(integral_constant<NT>) for nt in 1..MAX register tiles of 16 ring neighbours; any other nt launches nothing ----
template <int MAX, class F> static int nt_dispatch(int nt, F &&f) {
#define NT_CASE(N_) case N_: if constexpr (N_ <= MAX) return f(std::integral_constant<int, N_>{}); else return 0;
    switch (nt) { NT_CASE(1) NT_CASE(2) NT_CASE(3) NT_CASE(4) NT_CASE(5) NT_CASE(6) NT_CASE(7) NT_CASE(8) default: return 0; }
#undef NT_CASE
}
#define NT_OF(c) decltype(c)::value

static int solve_launch(cnmfe_ctx *ctx, Patch *P, const CovTab &tab, const BgGeom &g, const double *rowsum, const unsigned char *act, int nt, int probe, const double *fill) {
    int *dErr = nullptr;
    RET(ctx_errflag(ctx, &dErr));
    // one wave per pixel, the matrix in MFMA accumulator tiles (ring_solve.hpp).  Measured and removed (profiles/r02/solve_ab_c3.txt): the
    // panel-blocked LDS solver (22.5 ms against 8.0) and the looped-block-column variant (10.6 ms: it spills ~200 tile registers)
    return nt_dispatch<8>(nt, [&](auto c) -> int {
        LAUNCH(ctx, "bg_ring_solve", (k_ring_solve5<NT_OF(c)>), dim3((unsigned)P->d), dim3(64), 0, tab, g, P->ring_dr.as<int>(), P->ring_dc.as<int>(), rowsum, act, P->W.as<float>(), dErr, probe, (const int *)nullptr, fill);
        return 0; });
}

// ---- the rules the fit, bg_reserve and vproj.hip share: one copy each ----
int fits_leaving(const DevBuf &b, size_t bytes, bool *fits, bool quarter) {
    *fits = true;
    if (b.cap >= bytes) return 0;
    size_t fr = 0, tot = 0; CK(hipMemGetInfo(&fr, &tot));
    *fits = fr >= bytes + std::max((size_t)8 << 30, quarter ? tot / 4 : (size_t)0);
    return 0;
}
// the frame stride of a fit with projection (fit_ring_model.m:84-87): k = floor(T / min(T, 100 pmax)); pmax starts at p and only grows
static int fit_stride(int64_t T, int pmax) { return (int)std::max<int64_t>(1, T / std::max<int64_t>(1, std::min<int64_t>(T, (int64_t)pmax * 100))); }
// round 5 (gram_i8.hpp): a Gram over Tp frames on the int8 matrix pipe, exact up to a 32-bit quantisation of the data (option gram_i8, default 1; int32 range)
static bool gram_i8_ok(cnmfe_ctx *ctx, int64_t Tp) { return ctx->opt("gram_i8", 1) != 0 && Tp <= 24576; }
// the digit planes of the video stay resident with a patch whose fits use every frame (win_proj_i8.hpp) ...
static bool planes_wanted(cnmfe_ctx *ctx, const Patch *P, int kstride) { return kstride == 1 && !P->derived && ctx->opt("win_i8", 1) != 0; }
// ... and such a fit's window projection runs out of them (a strided fit keeps the fp64 window kernel)
static bool win_i8_applies(cnmfe_ctx *ctx, const Patch *P, int kstride) { return P->dig_valid && kstride == 1 && P->T <= 24576 && ctx->opt("win_i8", 1) != 0; }
// the packed systems of the ring solve (ring_solve_packed.hpp): 43 KB per pixel at p = 96
static bool pack_wanted(cnmfe_ctx *ctx, int nt) { return ctx->opt("solve_packed", 1) != 0 && nt >= 1 && nt <= 8; }
static size_t sys_bytes_of(int64_t d, int nt) { return (size_t)d * ((size_t)(nt * (nt + 1) / 2) * 256 + 16 * nt) * sizeof(double); }

// ---- launch helpers: the fit and win_i8_table go through them ----
// digits of the centred traces for the int8 window projection (gram: and their K x K Gram matrix, which k_win_fix then takes G from)
static int trace_gram(cnmfe_ctx *ctx, const float *dCc, int64_t ldc, int K, int64_t T) {
    RET(ctx->gk.ensure((size_t)K * K * sizeof(double)));
    LAUNCH(ctx, "bg_trace_gram", k_trace_gram, dim3((unsigned)(((K + 15) >> 4) * (((K + 15) >> 4) + 1) / 2)), dim3(64 * TG_W), 0, dCc, ldc, T, K, ctx->gk.as<double>());
    return 0;
}
static int trace_digits(cnmfe_ctx *ctx, const char *name, const float *dCc, int64_t ldc, int K, int64_t T, int64_t T16, bool gram) {
    RET(ctx->tdig.ensure((size_t)K * T16 * 4 * sizeof(uint4))); RET(ctx->tscale.ensure((size_t)K * sizeof(double)));
    if (gram) RET(ctx->gk.ensure((size_t)K * K * sizeof(double)));
    LAUNCH(ctx, name, k_trace_dig, dim3(K), dim3(256), 0, dCc, ldc, T, T16, ctx->tdig.as<uint4>(), ctx->tscale.as<double>());
    return gram ? trace_gram(ctx, dCc, ldc, K, T) : 0;
}
// round 5 (win_proj_i8.hpp): the window projection on the int8 matrix pipe out of the resident digit planes, one work item per (block, pair of trace groups)
// (in two steps: the upload of the work items, then the launch -- a fit that forks its side stream does so between them, with every upload of the compute stream sent)
static int win_proj_i8_items(cnmfe_ctx *ctx, const std::vector<int> &lst_ptr, const std::vector<int> &blall, size_t *nitems) {
    static thread_local std::vector<int> items;
    plan::win_i8_items(blall, lst_ptr, items);
    *nitems = items.size();
    return to_dev(ctx, ctx->win_items, items);
}
static int win_proj_i8_go(cnmfe_ctx *ctx, Patch *P, const char *name, size_t nitems, const int *dLp, const int *dLk, int nsg, double *dUt, int64_t ut_stride) {
    if (!nitems) return 0;
    const int64_t T16 = P->dig_T16;
#define WPI8_GO(V0_) LAUNCH(ctx, name, k_win_proj_i8<V0_>, dim3((unsigned)(nitems * nsg)), dim3(512), 0, P->dig.as<uint4>(), T16, P->dig_sc.as<double>(), ctx->tdig.as<uint4>(), \
                            ctx->tscale.as<double>(), dLp, dLk, ctx->win_items.as<int>(), nsg, dUt, ut_stride)
    if (win_planes3(ctx, T16)) WPI8_GO(1); else WPI8_GO(0);
#undef WPI8_GO
    return 0;
}
static int win_proj_i8_launch(cnmfe_ctx *ctx, Patch *P, const char *name, const std::vector<int> &lst_ptr, const std::vector<int> &blall, const int *dLp, const int *dLk, int nsg,
                              double *dUt, int64_t ut_stride) {
    size_t nitems = 0;
    RET(win_proj_i8_items(ctx, lst_ptr, blall, &nitems));
    return win_proj_i8_go(ctx, P, name, nitems, dLp, dLk, nsg, dUt, ut_stride);
}
// the digit planes of g's frames (gram_i8.hpp): the resident video minus da's footprints -> scales digs, planes digp; nchunk != nullptr: and the row sums per frame
// chunk in dig_rspart (*nchunk of them, reduced by k_rs_reduce)
static int build_digits(cnmfe_ctx *ctx, Patch *P, const BgGeom &g, const DigA &da, double *digs, uint4 *digp, int *nchunk) {
    const int nblk = g.nbr * g.nbc;
    RET(ctx->dig_smax.ensure((size_t)nblk * BLKPX * sizeof(unsigned)));
    CK(hipMemsetAsync(ctx->dig_smax.p, 0, (size_t)nblk * BLKPX * sizeof(unsigned), ctx->st()));
    const int tchunk16 = (int)((std::max<int64_t>(64, (g.Tpad + 15) / 16) + 15) & ~int64_t(15));
    const dim3 gd(nblk, (unsigned)((g.Tpad + tchunk16 - 1) / tchunk16));
    LAUNCH(ctx, "bg_dig_scale", k_dig_scale, gd, dim3(256), 0, P->Yc4.as<float4>(), P->Tc, g, da, tchunk16, ctx->dig_smax.as<unsigned>());
    if (nchunk) { RET(ctx->dig_rspart.ensure((size_t)gd.y * nblk * BLKPX * sizeof(double))); *nchunk = (int)gd.y; }
    LAUNCH(ctx, "bg_build_dig", k_build_dig, gd, dim3(256), 0, P->Yc4.as<float4>(), P->Tc, g, da, ctx->dig_smax.as<unsigned>(), digs, digp, tchunk16,
           nchunk ? ctx->dig_rspart.as<double>() : (double *)nullptr);
    return 0;
}

// The large buffers of the ring fit, allocated when the ring is set (cnmfe_ring_init: once per patch, after the upload) instead of inside the first fit: the
// video's covariance table, the context's working table, the tiled Bf and the window projection's partial sums -- 18 GB at the headline size.  A fit then
// queues its kernels without a hipMalloc in between (tens of milliseconds of the first iteration, and on some boxes the dispatch behind a fresh multi-GB
// allocation stalled for 0.5-0.8 s, profiles/r03/README.md).  Sizes follow the geometry only -- by the functions the fit itself decides with; a buffer that is
// already large enough is left alone.
int bg_reserve(cnmfe_ctx *ctx, Patch *P) {
    if (ctx->opt("gram_incremental", 1) == 0 || P->p <= 0) return 0;
    const plan::Reach reach = plan::ring_reach(P->dr.data(), P->dc.data(), P->p);
    if (!reach.ok) return 0;
    const bool i8 = gram_i8_ok(ctx, P->T);                   // (a stride-1 build: the first fit of most recordings)
    const BgGeom g = bg_geom(P, 1, i8);
    const int nblk = g.nbr * g.nbc, nt = (P->p + 15) / 16;
    const size_t tab = (size_t)plan::ring_pairs(P->nr_b, P->nc_b, P->roff, P->coff, P->nr, P->nc, reach.p_radius, reach.maxd, nullptr, nullptr) * BLKPX * BLKPX * sizeof(double);
    RET(P->cov_base.ensure(tab)); RET(P->rowsum_base.ensure((size_t)nblk * BLKPX * sizeof(double))); RET(ctx->cov.ensure(tab));
    RET(ctx->rowsum.ensure((size_t)nblk * BLKPX * sizeof(double))); RET(ctx->bf.ensure((size_t)nblk * g.Tpad * BLKPX * sizeof(float)));
    RET(ctx->inc[6].ensure((size_t)plan::win_segments(nblk) * nblk * WIN_NLB * WIN_NLB * sizeof(double)));      // (the segments of a fit with every block on a list; one with fewer listed blocks takes more and grows it)
    bool fits = false;
    if (pack_wanted(ctx, nt) && P->sys.cap < sys_bytes_of(P->d, nt)) {
        RET(fits_leaving(P->sys, sys_bytes_of(P->d, nt), &fits));
        if (fits) { P->drop_systems(); RET(P->sys.ensure(sys_bytes_of(P->d, nt))); }
    }
    // round 5: the two further copies of the video (digit planes of the window projection, the temporal projection's read-order copy) under the rule their builders
    // apply -- one more video's worth each, only if that leaves 8 GB free.  Allocated HERE, while the caller sets its patches up: a fresh 10 GB hipMalloc takes 0.3 ms
    // on most leases and 1-3 SECONDS on some (profiles/r05/first_iteration_stall.txt: one run in five, inside the first iteration's temporal projection)
    // (AHEAD of time only while a quarter of the device stays free: the buffers every patch's fit and updates must have are allocated later, and 64 patches
    //  reserving down to the builders' 8 GB left none for them -- tests/test_gpu_zconfigs.py::test_c5_whole_on_one_gpu; below that the builders decide as before)
    auto reserve = [&](DevBuf &b, size_t bytes) -> int { RET(fits_leaving(b, bytes, &fits, true)); return fits ? b.ensure(bytes) : 0; };
    if (P->derived) return 0;
    // (only a recording whose fits use every frame keeps digit planes)
    const bool planes = i8 && planes_wanted(ctx, P, fit_stride(P->T, P->p));
    if (planes) { RET(reserve(P->dig, (size_t)nblk * g.Tpad * BLKPX * sizeof(float))); RET(P->dig_sc.ensure((size_t)nblk * BLKPX * sizeof(double))); }
    if (ctx->opt("r1_virtual", 1) != 0) {
        // the temporal projection on the int8 pipe reads pixel-major planes instead of the read-order copy
        const kept::ProjOpts po = proj_opts(ctx);
        if (planes && po.i8 != 0) RET(reserve(P->digp, (size_t)nblk * g.Tpad * BLKPX * sizeof(float)));
        else if (po.tiled != 0) RET(reserve(P->yt4, (size_t)nblk * ((P->Tc + 15) >> 4) * 64 * 64 * sizeof(float4)));
    }
    return 0;
}

// ---- bg_fit_ring: the state its phases share, then the phases in the order they run ----
struct RingFit {
    cnmfe_ctx *ctx; Patch *P; int32_t K; const int64_t *A_colptr; const int32_t *A_rowidx; const float *A_val; const float *C; int c_order, b0_only; double thresh_outlier;
    HostTrace ht;
    bool outl, has_a, a_empty;                                 // ~isnan(thresh_outlier), :50; A has entries; isempty(A) -> A = ones(d,1), C = zeros(1,T) (:15-17): Bf = Y - Ymean, b0 = Ymean
    int64_t T, ldc = 4, nactive = 0;
    HostCSR csr;
    bool first_run = false; int pmax = 0, kstride = 1;
    BgGeom g; plan::Reach reach; int nblk = 0, nt = 0;
    // the plan (ring_plan.hpp)
    plan::BlockLists L; int npairs = 0, nwork = 0;            // (the pair / need / work / tile tables stay with the patch: Patch::RingTabs, fit_need_tables)
    // the path verdicts, each decided in one place.  fit_lists: incr = the incremental Gram (the video's table kept with the patch + this fit's corrections), build_base = this
    // fit builds that table, use_i8 = this fit's Gram (that table, or the direct Gram of Bf) runs on the int8 pipe, keep_pt = the window projection is the P = Yc Cc' table
    // the next spatial update wants.  fit_traces_up: trace_i8_done = the int8 window projection's trace digits and K x K Gram are queued.  fit_queue_projection: proj_queued;
    // win_i8 = it ran on the int8 pipe (k_win_fix takes G from the K x K matrix).  fit_pack: packed = the solve reads the packed systems.  fit_stage_windows: stage_ok
    bool incr = false, build_base = false, use_i8 = false, keep_pt = false, trace_i8_done = false, proj_queued = false, win_i8 = false, packed = false, stage_ok = false;
    // option fit_side (SideScope below).  fit_traces_up: gram_pending = the K x K trace Gram is still to be queued (the side scope takes it, or fit_queue_projection).
    // fit_side_setup: setup_done = the CSR rows, ind_active, b0 and slot_of are queued; stage_planned = so are the staged windows' metadata (stage_tot their length)
    bool gram_pending = false, setup_done = false, stage_planned = false; int64_t stage_tot = -1;
    int nsg = 1; int64_t ut_stride = 0, gb_stride = 0;
    uint4 *digp = nullptr; double *digs = nullptr;             // where the digit planes of this build live
    // device views
    DevBuf &dC, &dCc, &dCm, &dArow, &dAcol, &dAval, &dMisc, &dAsum, &dActive, &dPairs, &dPairOf, &dWork, &dNeed, &dTcnt, &dTl, &dLk, &dBl, &dUt, &dCsum, &dGb, *dLp, *dSlot;
    RingFit(cnmfe_ctx *c, Patch *p_) : ctx(c), P(p_), ht(c, "fit_ring"), dC(c->tmp[0]), dCc(c->tmp[1]), dCm(c->tmp[2]), dArow(c->tmp[3]), dAcol(c->tmp[4]), dAval(c->tmp[5]), dMisc(c->tmp[6]),
        dAsum(c->tmp[7]), dActive(c->tmp[8]), dPairs(p_->rt.dPairs), dPairOf(p_->rt.dPairOf), dWork(p_->rt.dWork), dNeed(p_->rt.dNeed), dTcnt(p_->rt.dTcnt), dTl(p_->rt.dTl), dLk(c->inc[1]),
        dBl(c->inc[3]), dUt(c->inc[4]), dCsum(c->inc[5]), dGb(c->inc[6]), dLp(&c->inc[0]), dSlot(&c->inc[2]) {}
    const int *arow() const { return has_a ? dArow.as<int>() : nullptr; }
    CovTab covtab() const { CovTab t{}; t.cov = ctx->cov.as<double>(); t.pair_of = dPairOf.as<int>(); t.nbr = g.nbr; t.nbc = g.nbc; t.maxd = reach.maxd; t.nrel = reach.nrel; return t; }
};
static thread_local std::vector<int> fit_nbox;                 // 4 per neuron: first / last row, first / last column of its footprint in the block region

static int fit_traces_up(RingFit &f) {
    cnmfe_ctx *ctx = f.ctx; Patch *P = f.P;
    if (!f.has_a) return 0;
    RET(upload_centered(ctx, f.dC, f.C, f.K, f.T, f.c_order, f.dCc, f.dCm, &f.ldc));
    // win_proj_i8.hpp: what depends on the traces alone goes out NOW -- the host's footprint block lists (0.2 ms at the headline size) are built underneath it
    // instead of in front of an idle GPU (the stride is not known yet: a fit that turns out to use another than the table in place has queued 0.1 ms for nothing)
    if (!f.outl && ctx->opt("gram_incremental", 1) != 0 && win_i8_applies(ctx, P, P->base_valid ? P->base_kstride : 1)) {
        // (fit_side: the K x K Gram waits until the fit knows whether its side scope runs -- the projection reads the digits only)
        f.gram_pending = ctx->opt("fit_side", 1) != 0 && ctx->lanes.empty();
        RET(trace_digits(ctx, "bg_trace_dig", f.dCc.as<float>(), f.ldc, f.K, f.T, P->dig_T16, !f.gram_pending));
        f.trace_i8_done = true;
    }
    return 0;
}
static int fit_trace_gram(RingFit &f) {
    if (!f.gram_pending) return 0;
    f.gram_pending = false;
    return trace_gram(f.ctx, f.dCc.as<float>(), f.ldc, f.K, f.T);
}
// the CSR rows of A (b0, ind_active, the table corrections): built AFTER the window projection is queued when that can go first
static int fit_upload_csr(RingFit &f) {
    if (!f.has_a) return 0;
    csc_to_csr(f.P->d_b, f.K, f.A_colptr, f.A_rowidx, f.A_val, f.csr);
    RET(to_dev(f.ctx, f.dArow, f.csr.rowptr)); RET(to_dev(f.ctx, f.dAcol, f.csr.col)); RET(to_dev(f.ctx, f.dAval, f.csr.val));
    return 0;
}
// ---- b0 (:44) ----
static int fit_b0(RingFit &f, const BgGeom &g) {
    LAUNCH(f.ctx, "bg_b0", k_b0, dim3((unsigned)((f.P->d + 255) / 256)), dim3(256), 0, f.P->ymean_d.as<double>(), g, f.arow(), f.dAcol.as<int>(), f.dAval.as<float>(), f.dCm.as<double>(),
           f.P->b0.as<double>());
    return 0;
}
// ---- first-run test (:25), frame stride (:84-87), geometry ----
static int fit_geometry(RingFit &f, int with_projection) {
    // first run: row 1 of W_old has exactly two distinct values (0 and 1/count).  Both questions about W_old were answered behind the call that produced it
    // (ring_stats_enqueue): no drain of the stream here, so with several patches per context the host sets up patch m + 1 while the GPU still solves patch m.
    RET(ring_stats_get(f.ctx, f.P, &f.pmax, &f.first_run));
    RET(f.dMisc.ensure(64));
    f.ht.mark("first_run + pmax");
    // with a threshold the frames are SELECTED instead (:62-67) and nmax = nnz(ind_frames) = size(Bf, 2) makes k = 1 at :84-85 (also when nmax >= T, where nk = min(T, nmax) = T)
    f.kstride = with_projection && !f.outl ? fit_stride(f.T, f.pmax) : 1;
    f.g = bg_geom(f.P, f.kstride);
    f.reach = plan::ring_reach(f.P->dr.data(), f.P->dc.data(), f.P->p);
    f.nblk = f.g.nbr * f.g.nbc; f.nt = (f.P->p + 15) / 16;
    if (!f.reach.ok) return fail(CNMFE_EUNSUPPORTED, "fit_ring_model: ring offsets up to %d pixels (the block-pair table covers <= 24)", f.reach.p_radius);
    return 0;
}
// ---- incremental Gram (k_win_proj / k_cov_correct): per 16x16 block the footprints with a pixel within maxd blocks of it; which table this fit uses or builds ----
static void fit_lists(RingFit &f) {
    cnmfe_ctx *ctx = f.ctx; Patch *P = f.P;
    static thread_local std::vector<int> pair_blk, k_ptr;
    f.incr = !f.outl && ctx->opt("gram_incremental", 1) != 0 && f.K < 32768;   // the clipped Bf is not linear in the video: direct Gram   // (derived low-resolution patches of bg_ssub included: their video is built once)
    if (f.incr) {
        plan::footprint_blocks(f.K, f.A_colptr, f.A_rowidx, P->nr_b, f.g.nbr, f.g.nbc, f.reach.maxd, pair_blk, k_ptr, fit_nbox);
        f.incr = plan::block_lists(f.nblk, f.K, pair_blk.data(), k_ptr.data(), f.L);            // (denser than the window kernel is built for: direct Gram)
    }
    if (f.incr && P->base_valid && P->base_kstride != f.kstride) {
        // the table in place is of another stride: it moves to the second slot, and what that slot held -- the table of THIS stride, if the recording
        // alternates -- comes forward (otherwise its memory is where the new table is built)
        P->cov_base.swap(P->cov_base_alt); P->rowsum_base.swap(P->rowsum_base_alt);
        std::swap(P->base_valid, P->base_alt_valid); std::swap(P->base_kstride, P->base_alt_kstride);
        P->sys.swap(P->sys_alt); std::swap(P->sys_valid, P->sys_alt_valid);          // (the packed systems belong to their table)
        P->drop_inverses();                                                          // (and the inverses to the packed systems)
    }
    f.build_base = f.incr && !(P->base_valid && P->base_kstride == f.kstride);
    if (f.build_base) P->drop_systems();
    f.ht.mark("footprint block lists");
    // the outlier branch (a clipped, frame-selected Bf) keeps the fp64 Gram kernel
    f.use_i8 = (f.build_base || !f.incr) && !f.outl && gram_i8_ok(ctx, f.g.Tp);
    geom_frames(f.g, f.g.Tp, f.use_i8);
    // keep_pt: all frames, the block's neurons, the same centred traces -- the raw sums are kept with the patch, and so are the lists that index them (then the fit
    // works out of the patch's copies)
    f.keep_pt = f.incr && f.has_a && f.kstride == 1 && !P->derived && !(f.b0_only & 2) && ctx->opt("r1_virtual", 1) != 0;
    if (f.keep_pt) { f.dLp = &P->pt_lp; f.dSlot = &P->pt_slot; P->pt_valid = false; }      // (until the new table is queued)
}
// ---- option fit_side: the fit's set-up on a second stream, beside the window projection ----
// A steady-state fit (the video's table exists: incr && has_a && !build_base) queues its 1.5 ms window projection first.  What follows up to k_win_fix -- the trace
// sums and the K x K trace Gram, the CSR rows of A, sum(A, 2), ind_active and its count, b0, slot_of, the staged windows' metadata -- reads nothing the projection
// writes and writes nothing it reads (the buffer table: DESIGN.md section 3, B1 / B2), and is a dozen latency-bound dispatches the compute stream would run one after
// the other behind it.  The scope puts them on the context's side stream:
//   fork()   every held-back upload of the compute stream sent, the error word in place, an event recorded on the compute stream; the side stream waits for it
//            -- and with it for everything queued earlier (the updates that used the same scratch)
//   enter()  the side stream takes the compute stream's place in the context: launches, held-back uploads (k_pin_copy) and the pinned arena's half-switch events
//            all go through cnmfe_ctx::st(), so they follow without knowing (what the lanes do with a whole scratch set)
//   leave()  the side stream's held-back uploads sent, an event recorded on it, the streams swapped back, the compute stream waits for the event
// fit_side = 1: fork, projection on the compute stream, enter .. leave -- the set-up runs under the projection.  2: fork, enter .. leave, THEN the projection: the same
// streams and code with nothing concurrent (tests; a wrong stream shows in both, a hazard of the overlap in 1 only).  0: one stream, the order of before.
// Between fork and leave the compute stream is given the projection's launches and nothing else: no upload, no event of the arena.
// (the scope itself: common.hpp, SideScope -- fork / enter / leave here; its second way to start, behind a recorded event, serves option ring_side in resid.hip)
// which way this fit goes (0: no side scope).  lanes > 1: every lane is a stream of its own already, and the patches' fits overlap each other
static int fit_side_mode(const RingFit &f) {
    const int64_t m = f.ctx->opt("fit_side", 1);
    return (m == 1 || m == 2) && f.ctx->lanes.empty() && f.incr && f.has_a && !f.build_base ? (int)m : 0;
}
static int fit_side_setup(RingFit &f);

// ---- the window projection: it needs the footprint lists and the traces, nothing else, and takes 5 ms at the headline size ----
static int fit_queue_projection(RingFit &f, int side = 0) {
    cnmfe_ctx *ctx = f.ctx; Patch *P = f.P; const BgGeom &g = f.g;
    SideScope sc(ctx);
    RET(to_dev(ctx, *f.dLp, f.L.lst_ptr)); RET(to_dev(ctx, f.dLk, f.L.lst_k)); RET(to_dev(ctx, f.dBl, f.L.blall)); RET(f.dCsum.ensure((size_t)f.K * sizeof(double)));
    if (!side) LAUNCH(ctx, "bg_trace_subsum", k_trace_subsum, dim3(f.K), dim3(256), 0, f.dCc.as<float>(), f.ldc, g.Tp, g.kstride, f.dCsum.as<double>());
    const int nb_ = (int)f.L.blall.size(), nbig = (int)f.L.blk_nt[3].size();                    // blall starts with the longest lists
    f.nsg = plan::win_segments(nb_);
    f.ut_stride = (int64_t)std::max<size_t>(1, f.L.lst_k.size()) * BLKPX; f.gb_stride = (int64_t)f.nblk * WIN_NLB * WIN_NLB;
    RET(f.dUt.ensure((size_t)f.nsg * f.ut_stride * sizeof(double))); RET(f.dGb.ensure((size_t)f.nsg * f.gb_stride * sizeof(double)));
    const int *dLp = f.dLp->as<int>(), *dLk = f.dLk.as<int>(), *dBl = f.dBl.as<int>();
    f.win_i8 = win_i8_applies(ctx, P, g.kstride);
    size_t nitems = 0;
    if (f.win_i8) {
        // (the first fit of a patch, or a fit back at stride 1: the digit planes did not exist, or were not this stride's, when the traces went up)
        if (!f.trace_i8_done) { f.gram_pending = side != 0; RET(trace_digits(ctx, "bg_trace_dig", f.dCc.as<float>(), f.ldc, f.K, f.T, P->dig_T16, !f.gram_pending)); f.trace_i8_done = true; }
        if (!side) RET(fit_trace_gram(f));
        RET(win_proj_i8_items(ctx, f.L.lst_ptr, f.L.blall, &nitems));
    }
    if (side) RET(sc.fork());
    if (side == 2) { RET(sc.enter()); RET(fit_side_setup(f)); RET(sc.leave()); }
    if (f.win_i8) {
        // the same sums out of the resident digit planes; G = Cc Cc' once, K x K
        // (round 6 ran a strided fit here too -- planes of every frame, trace digits zeroed on the skipped frames: correct, and no faster than the fp64 kernel on
        //  patches of 128 x 128, which reads its 2 GB at 5.5 TB/s already, while the K x K trace Gram became a kernel of its own: profiles/r06/c5shard_i8.txt)
        RET(win_proj_i8_go(ctx, P, "bg_win_proj", nitems, dLp, dLk, f.nsg, f.dUt.as<double>(), f.ut_stride));
    } else if (g.kstride == 1 || g.kstride == 2 || g.kstride == 4)
        RET(win_proj4_launch(ctx, "bg_win_proj", P, g, f.dCc.as<float>(), f.ldc, dLp, dLk, dBl, nbig, nb_, f.nsg, f.dUt.as<double>(), f.ut_stride, f.dGb.as<double>(), f.gb_stride));
    else
        LAUNCH(ctx, "bg_win_proj", k_win_proj, dim3((unsigned)(nb_ * f.nsg)), dim3(256), 0, P->Yc4.as<float4>(), g, f.dCc.as<float>(), f.ldc, dLp, dLk, dBl, f.nsg, f.dUt.as<double>(), f.ut_stride,
               f.dGb.as<double>(), f.gb_stride);
    f.proj_queued = true;
    if (side == 1) { RET(sc.enter()); RET(fit_side_setup(f)); RET(sc.leave()); }
    return 0;
}
// ---- ind_active (:25-29), b0 (:44) ----
static int fit_active_b0(RingFit &f) {
    cnmfe_ctx *ctx = f.ctx; Patch *P = f.P;
    RET(f.dActive.ensure(P->d));
    f.nactive = P->d;
    if (f.first_run) { CK(hipMemsetAsync(f.dActive.p, 1, P->d, ctx->st())); } else {
        // isempty(A) -> A = ones(d,1) (:14-16).  Bit 1 of b0_only: the reference passes A = [] because it subtracted A*C itself (bg_ssub > 1)
        // (sum(A, 2) out of the CSR rows that are on the device by now: k_asum)
        const bool ones = f.a_empty || (f.b0_only & 2);
        RET(f.dAsum.ensure((size_t)P->d_b * sizeof(float)));
        LAUNCH(ctx, "bg_asum", k_asum, dim3((unsigned)((P->d_b + 255) / 256)), dim3(256), 0, !ones && f.has_a ? f.dArow.as<int>() : (const int *)nullptr, f.dAval.as<float>(), ones ? 1.0f : 0.0f,
               (int64_t)P->d_b, f.dAsum.as<float>());
        CK(hipMemsetAsync(f.dMisc.p, 0, 64, ctx->st()));
        LAUNCH(ctx, "bg_active", k_active, dim3((unsigned)((P->d + 255) / 256)), dim3(256), 0, P->W.as<float>(), f.g,
               P->ring_dr.as<int>(), P->ring_dc.as<int>(), f.dAsum.as<float>(), f.dActive.as<unsigned char>(), f.dMisc.as<int>());
        // the count is only reported (info[2]): it lands in pinned memory and is read if the call ends with a drain anyway (b0_out)
        CK(hipMemcpyAsync((char *)P->stat_host + 8, f.dMisc.p, sizeof(int), hipMemcpyDeviceToHost, ctx->st()));
        f.nactive = -1;
    }
    return fit_b0(f, f.g);
}
// ---- pair list, needed sub-tiles, work and tile lists (ring_plan.hpp) and their uploads; the working table ----
// (pixels that are not active keep their weights: the solve kernel skips them; a patch without any costs the sweep of its tables)
static int fit_pair_tables(RingFit &f) {
    cnmfe_ctx *ctx = f.ctx; Patch *P = f.P;
    // the tables follow the block geometry and the ring offsets alone: under an unchanged key the fit takes the pair count from the patch and leaves the tables to
    // whichever of its kernels reads them (fit_need_tables) -- in a steady-state packed fit none does
    Patch::RingTabs &rt = P->rt;
    const int geo[8] = {(int)P->nr_b, (int)P->nc_b, (int)P->roff, (int)P->coff, (int)P->nr, (int)P->nc, f.reach.p_radius, f.reach.maxd};
    if (!(rt.keyed && std::equal(geo, geo + 8, rt.geo) && rt.dr == P->dr && rt.dc == P->dc)) {
        rt.keyed = rt.built = false;
        rt.npairs = plan::ring_pairs(geo[0], geo[1], geo[2], geo[3], geo[4], geo[5], geo[6], geo[7], nullptr, nullptr);
        std::copy(geo, geo + 8, rt.geo); rt.dr = P->dr; rt.dc = P->dc; rt.keyed = true;
    }
    f.npairs = rt.npairs;
    f.ht.mark("pair / need / work tables");
    const size_t cov_bytes = (size_t)f.npairs * BLKPX * BLKPX * sizeof(double);
    RET(ctx->cov.ensure(cov_bytes));
    if (ctx->opt("debug", 0)) CK(hipMemsetAsync(ctx->cov.p, 0xff, cov_bytes, ctx->st()));   // NaN-poison skipped sub-tiles
    f.ht.mark("tile lists + uploads (sync)");
    // incremental: the table of the video alone is built once and kept with the patch; later fits skip B1 / B2a entirely
    if (f.incr) {
        RET(P->cov_base.ensure(cov_bytes));
        if (f.build_base && ctx->opt("debug", 0)) CK(hipMemsetAsync(P->cov_base.p, 0xff, cov_bytes, ctx->st()));
    }
    return 0;
}
// the tables themselves, for a fit one of whose kernels reads them (the table builds: pairs, work, tile lists; k_win_codes: pair_of; k_cov_correct: pairs, needmask):
// computed and uploaded when the key changed since they last were, into buffers of the patch's own -- the context's scratch is anybody's between two fits
static int fit_need_tables(RingFit &f) {
    cnmfe_ctx *ctx = f.ctx; Patch *P = f.P; Patch::RingTabs &rt = P->rt;
    if (!rt.built) {
        plan::ring_pairs(rt.geo[0], rt.geo[1], rt.geo[2], rt.geo[3], rt.geo[4], rt.geo[5], rt.geo[6], rt.geo[7], &rt.pairs, &rt.pair_of);
        plan::ring_tables(rt.pairs, f.reach.maxd, f.reach.p_radius, P->dr.data(), P->dc.data(), P->p, rt.tabs);
        rt.nwork = (int)rt.tabs.work.size();
        RET(to_dev(ctx, rt.dPairs, rt.pairs)); RET(to_dev(ctx, rt.dPairOf, rt.pair_of)); RET(to_dev(ctx, rt.dWork, rt.tabs.work)); RET(to_dev(ctx, rt.dNeed, rt.tabs.needmask));
        RET(to_dev(ctx, rt.dTcnt, rt.tabs.tcnt)); RET(to_dev(ctx, rt.dTl, rt.tabs.tlist));
        rt.built = true;
    }
    f.nwork = rt.nwork;
    return 0;
}
// ---- B1: Bf tiled (fp32, or digit planes for the int8 Gram) and its row sums rsT ----
static int fit_build_bf(RingFit &f, DevBuf &rsT) {
    cnmfe_ctx *ctx = f.ctx; Patch *P = f.P; const BgGeom &g = f.g; const int nblk = f.nblk;
    const bool has_a_bf = f.has_a && !f.incr;
    RET(ctx->bf.ensure((size_t)nblk * g.Tpad * BLKPX * sizeof(float))); RET(rsT.ensure((size_t)nblk * BLKPX * sizeof(double)));
    if (!f.use_i8) {
        const int tchunk = (int)((std::max<int64_t>(64, (g.Tpad + 15) / 16) + 7) & ~int64_t(7));
        LAUNCH(ctx, "bg_build_bf", k_build_bf, dim3(nblk, (unsigned)((g.Tpad + tchunk - 1) / tchunk)), dim3(256), 0, P->Yc4.as<float4>(), P->Tc, g,
               has_a_bf ? f.dArow.as<int>() : nullptr, f.dAcol.as<int>(), f.dAval.as<float>(), f.dCc.as<float>(), f.ldc, ctx->bf.as<float>(), tchunk, rsT.as<double>());
        return 0;
    }
    // the VIDEO's planes stay resident with the patch (the fits' window projection reads them, win_proj_i8.hpp) when one more video's worth of memory
    // leaves 8 GB free and the stride is 1; otherwise, and for the direct Gram of Bf, in the context's scratch
    const size_t dbytes = (size_t)nblk * g.Tpad * BLKPX * sizeof(float), sbytes = (size_t)nblk * BLKPX * sizeof(double);
    bool resident = f.incr && planes_wanted(ctx, P, f.kstride);
    if (resident) RET(fits_leaving(P->dig, dbytes, &resident));
    if (resident) {
        RET(P->dig.ensure(dbytes)); RET(P->dig_sc.ensure(sbytes));
        f.digp = P->dig.as<uint4>(); f.digs = P->dig_sc.as<double>();
        P->dig_T16 = g.Tpad >> 4; P->dig_valid = true; P->digp_valid = false;
    } else {
        RET(ctx->dig_scale.ensure(sbytes));
        f.digp = ctx->bf.as<uint4>(); f.digs = ctx->dig_scale.as<double>();
    }
    int nchunk = 0;
    RET(build_digits(ctx, P, g, DigA{has_a_bf ? f.dArow.as<int>() : nullptr, f.dAcol.as<int>(), f.dAval.as<float>(), f.dCc.as<float>(), f.ldc}, f.digs, f.digp, &nchunk));
    LAUNCH(ctx, "bg_rs_reduce", k_rs_reduce, dim3((unsigned)nblk), dim3(256), 0, ctx->dig_rspart.as<double>(), nchunk, (int64_t)nblk * BLKPX, rsT.as<double>());
    // round 6: a fit on every kstride-th frame (T > 100 pmax: BASELINE configs[4], T = 20000) built the planes of ITS frames above, in the scratch, for the table.
    // The planes the spatial update's table and the temporal projection read hold EVERY frame and are built here, once per recording, under the same memory
    // rule (until round 5 a strided recording ran both on the fp64 pipe: 2.9-3.0 ms each for a rank's share of configs[4], profiles/r05/bench_c5shard_v3.json;
    // 2.5-2.6 ms now -- at that patch size all three video passes move their bytes at 5.5 TB/s whatever the pipe)
    // (round 6, late: up to I8_SEG_FRAMES * 16 frames -- the projections that contract over FRAMES keep every int32 sum inside one frame segment of at most
    //  I8_SEG_FRAMES frames, vproj.hip; the temporal projection contracts over pixels and has no such limit)
    if (f.incr && f.kstride > 1 && !has_a_bf && f.T <= (int64_t)I8_SEG_FRAMES * 16 && planes_wanted(ctx, P, 1)) {
        BgGeom g1 = g; g1.kstride = 1; geom_frames(g1, f.T, true);
        bool ok = false;
        RET(fits_leaving(P->dig, (size_t)nblk * g1.Tpad * BLKPX * sizeof(float), &ok));
        if (ok) {
            RET(P->dig.ensure((size_t)nblk * g1.Tpad * BLKPX * sizeof(float))); RET(P->dig_sc.ensure(sbytes));
            RET(build_digits(ctx, P, g1, DigA{nullptr, nullptr, nullptr, nullptr, 0}, P->dig_sc.as<double>(), P->dig.as<uint4>(), nullptr));
            P->dig_T16 = g1.Tpad >> 4; P->dig_valid = true; P->digp_valid = false;
        }
    }
    return 0;
}
// ---- :50-56 clip, :60-67 frame selection (the outlier branch: Bf is rewritten in place, g's frames become the kept ones) ----
static int fit_outlier_frames(RingFit &f) {
    cnmfe_ctx *ctx = f.ctx; Patch *P = f.P; BgGeom &g = f.g; const int64_t T = f.T;
    const size_t bfbytes = (size_t)f.nblk * g.Tpad * BLKPX * sizeof(float);
    RET(ctx->bf2.ensure(bfbytes)); RET(ctx->outl_cnt.ensure((size_t)T * sizeof(int)));
    CK(hipMemcpyAsync(ctx->bf2.p, ctx->bf.p, bfbytes, hipMemcpyDeviceToDevice, ctx->st()));
    CK(hipMemsetAsync(ctx->outl_cnt.p, 0, (size_t)T * sizeof(int), ctx->st()));
    LAUNCH(ctx, "bg_outlier_clip", k_outlier_clip, dim3((unsigned)((P->d + 255) / 256), (unsigned)(g.Tpad >> 2)), dim3(256), 0, ctx->bf.as<float4>(),
           ctx->bf2.as<float4>(), g, P->ring_dr.as<int>(), P->ring_dc.as<int>(), P->W.as<float>(), P->sn_b.as<float>(), f.thresh_outlier,
           ctx->outl_cnt.as<int>());
    std::vector<int> sel;
    const int64_t nmax = (int64_t)f.pmax * 100;                     // :61
    if (nmax < T) {                                                 // :62
        std::vector<int> cnt((size_t)T);
        CK(hipMemcpyAsync(cnt.data(), ctx->outl_cnt.p, (size_t)T * sizeof(int), hipMemcpyDeviceToHost, ctx->st()));
        CK(hipStreamSynchronize(ctx->st()));
        const double qv = matlab_quantile(cnt, (double)nmax / (double)T);   // :64
        for (int64_t t = 0; t < T; ++t) if ((double)cnt[t] <= qv) sel.push_back((int)t);
    } else for (int64_t t = 0; t < T; ++t) sel.push_back((int)t);
    const int64_t Tpad_src = g.Tpad;
    geom_frames(g, (int64_t)sel.size(), false);
    RET(to_dev(ctx, ctx->outl_sel, sel));
    LAUNCH(ctx, "bg_select_frames", k_select_frames, dim3(f.nblk, (unsigned)std::min<int64_t>(64, std::max<int64_t>(1, g.Tpad >> 2))), dim3(256), 0,
           ctx->bf2.as<float>(), Tpad_src, ctx->bf.as<float>(), g.Tpad, ctx->outl_sel.as<int>(), g.Tp);
    CK(hipStreamSynchronize(ctx->st()));                           // `sel` is staged from this scope
    return 0;
}
// ---- B1 + B2a: the table this fit has to build -- the video's (kept with the patch) or the direct Gram of Bf (the context's working table) ----
static int fit_base_table(RingFit &f) {
    cnmfe_ctx *ctx = f.ctx; Patch *P = f.P; const BgGeom &g = f.g;
    DevBuf &covT = f.incr ? P->cov_base : ctx->cov, &rsT = f.incr ? P->rowsum_base : ctx->rowsum;
    RET(fit_need_tables(f));
    RET(fit_build_bf(f, rsT));
    if (f.outl) RET(fit_outlier_frames(f));
    if (g.bf4 < 2) LAUNCH(ctx, "bg_rowsum", k_rowsum, dim3(f.nblk), dim3(256), 0, ctx->bf.as<float>(), g.Tpad, rsT.as<double>(), g.bf4);
    const int nwg = (f.nwork + 7) / 8 * 8;                    // multiple of 8 for the XCD remap (extra workgroups exit)
    const size_t shmem = (size_t)G4_NBUF * G4_STAGE_F * sizeof(float);
    static bool attr4 = false, attr8 = false;
    if (!attr4) { CK(hipFuncSetAttribute((const void *)k_gram4, hipFuncAttributeMaxDynamicSharedMemorySize, (int)shmem)); attr4 = true; }
    if (f.use_i8) {
        if (!attr8) { CK(hipFuncSetAttribute((const void *)k_gram_i8, hipFuncAttributeMaxDynamicSharedMemorySize, GI_NBUF * GI_STAGE_B)); attr8 = true; }
        LAUNCH(ctx, "bg_gram_i8", k_gram_i8, dim3(nwg), dim3(512), (size_t)GI_NBUF * GI_STAGE_B, f.digp, g.Tpad >> 4, f.dPairs.as<int4>(), f.dWork.as<int>(), f.nwork,
               f.dTcnt.as<int>(), f.dTl.as<int>(), f.digs, covT.as<double>());
    } else
        LAUNCH(ctx, "bg_gram_f64", k_gram4, dim3(nwg), dim3(256), shmem, ctx->bf.as<float>(), g.Tpad, f.dPairs.as<int4>(), f.dWork.as<int>(), f.nwork,
               f.dTcnt.as<int>(), f.dTl.as<int>(), 0, covT.as<double>());
    if (f.incr) { P->base_valid = true; P->base_kstride = f.kstride; }
    return 0;
}
// the block-pair codes per window origin (k_win_codes): for the pack and for the table solve
static int fit_win_codes(RingFit &f) {
    const int woff = f.reach.woff, nwin = (f.g.nbr + 2 * woff) * (f.g.nbc + 2 * woff);
    RET(fit_need_tables(f));
    RET(f.ctx->wcodes.ensure((size_t)nwin * 256 * sizeof(int)));
    LAUNCH(f.ctx, "bg_win_codes", k_win_codes, dim3((unsigned)nwin), dim3(256), 0, f.dPairOf.as<int>(), f.g.nbr, f.g.nbc, woff, f.reach.maxd, f.reach.nrel, f.ctx->wcodes.as<int>());
    return 0;
}
// ---- packed systems (ring_solve_packed.hpp): the video's table re-laid once per pixel in the solve's register-tile order; the fits then apply the
// footprints' corrections in registers and neither sweep the table (k_cov_correct) nor gather from it.  Conditions: the incremental table,
// the memory, one launch (no split solve) ----
static int fit_pack(RingFit &f) {
    cnmfe_ctx *ctx = f.ctx; Patch *P = f.P; const int nt = f.nt;
    const double fillv[2] = {0.0, 1.0};                      // the fill values {0, 1} of missing neighbours, in global memory (ring_solve.hpp): constants, uploaded once
    if (!ctx->solve_fill.p) RET(to_dev(ctx, ctx->solve_fill, fillv, 2));
    f.packed = f.incr && pack_wanted(ctx, nt) && (int64_t)f.nblk * std::max(1, f.K) < (int64_t)1 << 31 && (int64_t)f.L.lst_k.size() * BLKPX < (int64_t)1 << 31;
    const size_t sys_bytes = sys_bytes_of(P->d, nt);
    if (!f.packed || (P->sys_valid && P->sys.cap >= sys_bytes)) return 0;
    RET(fits_leaving(P->sys, sys_bytes, &f.packed));         // (not worth the last gigabytes: the table path needs none of this)
    if (!f.packed) return 0;
    RET(P->sys.ensure(sys_bytes));
    RET(fit_win_codes(f));
    CovTab tb = f.covtab(); tb.cov = P->cov_base.as<double>(); tb.wcodes = ctx->wcodes.as<int>(); tb.woff = f.reach.woff;
    int *dErrP = nullptr;
    RET(ctx_errflag(ctx, &dErrP));
    RET(nt_dispatch<8>(nt, [&](auto c) -> int {
        LAUNCH(ctx, "bg_sys_pack", (k_sys_pack<NT_OF(c)>), dim3((unsigned)P->d), dim3(64), 0, tb, f.g, P->ring_dr.as<int>(), P->ring_dc.as<int>(), P->rowsum_base.as<double>(),
               (const unsigned char *)nullptr, (float *)nullptr, dErrP, 0, (const int *)nullptr, ctx->solve_fill.as<double>(), P->sys.as<double>());
        return 0; }));
    P->drop_inverses(); P->sys_valid = true;
    return 0;
}
// ---- round 6 (ring_solve_staged.hpp): U~ and A of every neuron as dense images over its footprint's bounding box dilated by the ring radius, and per list
// position the neuron's window: the solve samples them with index arithmetic instead of walking CSR rows and slot tables ----
static bool fit_stage_wanted(const RingFit &f) { return f.ctx->opt("solve_staged", 1) != 0 && f.P->nr_b < 32768 && f.P->nc_b < 32768; }
// (the host's part and the uploads: they depend on the footprints' boxes and the lists alone, so a fit that is sure of its packed systems plans in its side scope)
static int fit_stage_plan(RingFit &f) {
    cnmfe_ctx *ctx = f.ctx; Patch *P = f.P;
    static thread_local std::vector<int> nmeta, lmeta;
    const int64_t tot = f.stage_tot = plan::stage_windows(f.K, fit_nbox, f.L.lst_k, P->nr_b, P->nc_b, f.reach.p_radius, nmeta, lmeta);
    f.stage_planned = true;
    if (tot < 0) return 0;                                     // (a window too large: k_ring_solve6 serves this fit)
    RET(to_dev(ctx, ctx->stg[0], nmeta)); RET(to_dev(ctx, ctx->stg[1], lmeta));
    RET(ctx->stg[2].ensure((size_t)std::max<int64_t>(1, tot) * sizeof(double)));
    RET(ctx->stg[3].ensure((size_t)std::max<int64_t>(1, tot) * sizeof(float)));
    return 0;
}
static int fit_stage_windows(RingFit &f) {
    cnmfe_ctx *ctx = f.ctx;
    if (!(f.packed && fit_stage_wanted(f))) return 0;
    if (!f.stage_planned) RET(fit_stage_plan(f));
    if (f.stage_tot < 0) return 0;
    f.stage_ok = true;
    int *dErrW = nullptr;
    RET(ctx_errflag(ctx, &dErrW));
    LAUNCH(ctx, "bg_neuron_windows", k_nwin_build, dim3((unsigned)f.K), dim3(256), 0, ctx->stg[0].as<int>(), f.g, (int)f.K, f.dArow.as<int>(), f.dAcol.as<int>(), f.dAval.as<float>(),
           f.dLp->as<int>(), f.dSlot->as<short>(), f.dUt.as<double>(), ctx->stg[2].as<double>(), ctx->stg[3].as<float>(), dErrW);
    return 0;
}
// slot_of on the device: the inverse of the lists lst_ptr / lst_k that went up for the projection (the host's copy stays with the patch for the spatial update's reuse test)
static int fit_slot_table(RingFit &f) {
    const size_t bytes = (size_t)f.nblk * std::max(1, (int)f.K) * sizeof(short);
    RET(f.dSlot->ensure(bytes));
    CK(hipMemsetAsync(f.dSlot->p, 0xff, bytes, f.ctx->st()));
    LAUNCH(f.ctx, "bg_slot_table", k_slot_build, dim3((unsigned)f.nblk), dim3(64), 0, f.dLp->as<int>(), f.dLk.as<int>(), (int)f.K, f.dSlot->as<short>());
    return 0;
}
// what a steady-state fit queues between its window projection and k_win_fix without reading anything the projection writes (SideScope: on the side stream)
static int fit_side_setup(RingFit &f) {
    cnmfe_ctx *ctx = f.ctx; Patch *P = f.P;
    LAUNCH(ctx, "bg_trace_subsum", k_trace_subsum, dim3(f.K), dim3(256), 0, f.dCc.as<float>(), f.ldc, f.g.Tp, f.g.kstride, f.dCsum.as<double>());
    if (f.win_i8) RET(fit_trace_gram(f));
    RET(fit_upload_csr(f));
    f.ht.mark("A csr");
    RET(fit_active_b0(f));
    f.ht.mark("ind_active + b0");
    RET(fit_slot_table(f));
    // the staged windows' metadata, when the packed systems are in place already (then fit_pack has nothing to decide)
    if (f.incr && pack_wanted(ctx, f.nt) && P->sys_valid && P->sys.cap >= sys_bytes_of(P->d, f.nt) && (int64_t)f.nblk * std::max(1, f.K) < (int64_t)1 << 31 &&
        (int64_t)f.L.lst_k.size() * BLKPX < (int64_t)1 << 31 && fit_stage_wanted(f)) RET(fit_stage_plan(f));
    f.setup_done = true;
    return 0;
}
// ---- B2a': U~ on the blocks near footprints, then one sweep base -> cov (table path) or nothing (packed path: the solve corrects in registers) ----
static int fit_corrections(RingFit &f, const float *C, int c_order) {
    cnmfe_ctx *ctx = f.ctx; Patch *P = f.P; const BgGeom &g = f.g; const int K = (int)f.K;
    RET(ctx->rowsum.ensure((size_t)f.nblk * BLKPX * sizeof(double)));
    if (!f.has_a) {                                            // no footprints: Bf is the centred video itself
        if (!f.packed) CK(hipMemcpyAsync(ctx->cov.p, P->cov_base.p, (size_t)f.npairs * BLKPX * BLKPX * sizeof(double), hipMemcpyDeviceToDevice, ctx->st()));
        CK(hipMemcpyAsync(ctx->rowsum.p, P->rowsum_base.p, (size_t)f.nblk * BLKPX * sizeof(double), hipMemcpyDeviceToDevice, ctx->st()));
        return 0;
    }
    if (!f.proj_queued) RET(fit_queue_projection(f));          // (first fit of the patch: behind the video's table)
    if (!f.setup_done) RET(fit_slot_table(f));
    if (f.keep_pt) RET(P->pt_tab.ensure(std::max<size_t>(1, f.L.lst_k.size()) * BLKPX * sizeof(double)));
    LAUNCH(ctx, "bg_win_fix", k_win_fix, dim3((unsigned)f.L.blall.size(), WIN_NLB / WF_S), dim3(256), 0, g, K, f.dArow.as<int>(), f.dAcol.as<int>(), f.dAval.as<float>(), f.dLp->as<int>(),
           f.dSlot->as<short>(), f.dBl.as<int>(), f.nsg, f.dUt.as<double>(), f.ut_stride, f.dGb.as<double>(), f.gb_stride, f.keep_pt ? P->pt_tab.as<double>() : nullptr,
           f.win_i8 ? ctx->gk.as<double>() : (const double *)nullptr, f.dLk.as<int>());
    if (f.keep_pt) {
        P->pt_K = K; P->pt_lp_h = f.L.lst_ptr; P->pt_slot_h = f.L.slot_of;
        P->pt_gen = bound_rows_of(ctx, C, c_order, K, P->pt_rows) ? ctx->bound_gen : -1;
        P->pt_valid = true;
    }
    const int csplit = f.npairs >= 8192 ? 1 : f.npairs >= 4096 ? 2 : 4;      // (small patches: a pair's sweep is a long serial loop, one workgroup per pair leaves the chip idle)
    if (!f.packed) RET(fit_need_tables(f));
    if (!f.packed)
        LAUNCH(ctx, "bg_cov_correct", k_cov_correct, dim3((unsigned)f.npairs, (unsigned)csplit), dim3(256), 0, P->cov_base.as<double>(), ctx->cov.as<double>(), f.dPairs.as<int4>(),
               f.dNeed.as<unsigned short>(), g, K, f.dArow.as<int>(), f.dAcol.as<int>(), f.dAval.as<float>(), f.dLp->as<int>(), f.dSlot->as<short>(), f.dUt.as<double>());
    LAUNCH(ctx, "bg_rowsum_correct", k_rowsum_correct, dim3(f.nblk), dim3(256), 0, P->rowsum_base.as<double>(), ctx->rowsum.as<double>(), g,
           f.dArow.as<int>(), f.dAcol.as<int>(), f.dAval.as<float>(), f.dCsum.as<double>());
    return fit_stage_windows(f);
}
// ---- B2b on the packed systems: out of the cached inverses (ring_solve_inv.hpp), the staged windows (k_ring_solve8) or the CSR rows (k_ring_solve6) ----
static int fit_solve_packed(RingFit &f, const unsigned char *act, int probe) {
    cnmfe_ctx *ctx = f.ctx; Patch *P = f.P; const BgGeom &g = f.g; const int nt = f.nt;
    const int *dr = P->ring_dr.as<int>(), *dc = P->ring_dc.as<int>(); const double *sys = P->sys.as<double>(), *rowsum = ctx->rowsum.as<double>(); float *W = P->W.as<float>();
    const unsigned d = (unsigned)P->d;
    PackArgs pa{};
    if (f.has_a) {
        pa.arow = f.dArow.as<int>(); pa.acol = f.dAcol.as<int>(); pa.aval = f.dAval.as<float>(); pa.lst_ptr = f.dLp->as<int>(); pa.lst_k = f.dLk.as<int>();
        pa.slot_of = f.dSlot->as<short>(); pa.K = (int)f.K; pa.Ut = f.dUt.as<double>();
    }
    int *dErrS = nullptr;
    RET(ctx_errflag(ctx, &dErrS));
    // solve_inv: 0 off; 1 the inverses are built in front of a patch's SECOND fit with footprints (a recording fitted once never pays the build) at the ridge its
    // first fit left; 2 in front of the first  (off by default: in the steady-state iteration the ridge drifts every fit, the series takes 1-2 terms per pixel and
    // the fit is no faster than the factorising kernel -- DESIGN.md)
    const int inv_mode = (int)ctx->opt("solve_inv", 0);
    const size_t kinv_bytes = (size_t)P->d * (size_t)ri_stride(nt) * sizeof(double);
    bool inv_ok = inv_mode != 0 && f.has_a && nt <= 6 && !(probe & 7);
    if (inv_ok) RET(fits_leaving(P->kinv, kinv_bytes, &inv_ok));
    double *lam_arr = nullptr;
    if (inv_ok) {
        if (P->kinv_lam.cap < (size_t)P->d * sizeof(double)) { RET(P->kinv_lam.ensure((size_t)P->d * sizeof(double))); P->kinv_lam_valid = false; }
        RET(P->kinv_list.ensure(((size_t)2 * P->d + 4) * sizeof(int)));
        if (!P->kinv_lam_valid) { CK(hipMemsetAsync(P->kinv_lam.p, 0, (size_t)P->d * sizeof(double), ctx->st())); P->kinv_lam_valid = true; }
        lam_arr = P->kinv_lam.as<double>();
        if (!P->kinv_valid && (P->kinv_fits >= 1 || inv_mode >= 2)) {
            RET(P->kinv.ensure(kinv_bytes));
            RET(nt_dispatch<6>(nt, [&](auto c) -> int {
                LAUNCH(ctx, "bg_ring_inverse", (k_ring_inverse<NT_OF(c)>), dim3(d), dim3(64), 0, sys, g, dr, dc, P->rowsum_base.as<double>(), (const double *)lam_arr, P->kinv.as<double>());
                return 0; }));
            P->kinv_valid = true;
        }
        ++P->kinv_fits;
    }
    if (inv_ok && P->kinv_valid) {
        int *flist = P->kinv_list.as<int>(), *rlist = flist + P->d, *fcnt = flist + 2 * P->d;
        CK(hipMemsetAsync(fcnt, 0, 4 * sizeof(int), ctx->st()));
        InvArgs ia{};
        ia.kp = P->kinv.as<double>(); ia.sys = P->sys.as<double>(); ia.csum = f.dCsum.as<double>(); ia.lam_out = lam_arr;
        ia.flist = flist; ia.rlist = rlist; ia.fcnt = fcnt; ia.maxit = (int)ctx->opt("solve_inv_terms", 5);
        const unsigned nlist = (unsigned)std::min<int64_t>(P->d, 2048);
        return nt_dispatch<6>(nt, [&](auto c) -> int {
            LAUNCH(ctx, "bg_ring_solve", (k_ring_apply<NT_OF(c)>), dim3(d), dim3(64), 0, ia, pa, g, dr, dc, rowsum, act, W, dErrS, probe, (const int *)nullptr);
            LAUNCH(ctx, "bg_ring_solve_rest", (k_ring_solve6<NT_OF(c)>), dim3(d), dim3(64), 0, sys, pa, g, dr, dc, rowsum, (const unsigned char *)nullptr, W, dErrS, probe, (const int *)flist,
                   (const int *)fcnt, lam_arr);
            LAUNCH(ctx, "bg_ring_inverse_rest", (k_ring_inverse_list<NT_OF(c)>), dim3(nlist), dim3(64), 0, sys, g, dr, dc, P->rowsum_base.as<double>(), (const double *)lam_arr,
                   P->kinv.as<double>(), (const int *)rlist, (const int *)(fcnt + 3));
            return 0; });
    }
    if (f.has_a && f.stage_ok && nt <= 6) {
        StageArgs sg{f.dLp->as<int>(), ctx->stg[1].as<int>(), ctx->stg[2].as<double>(), ctx->stg[3].as<float>()};
        return nt_dispatch<6>(nt, [&](auto c) -> int {
            LAUNCH(ctx, "bg_ring_solve", (k_ring_solve8<NT_OF(c)>), dim3(d), dim3(64), 0, sys, sg, g, dr, dc, rowsum, act, W, dErrS, probe, (const int *)nullptr, lam_arr);
            return 0; });
    }
    return nt_dispatch<8>(nt, [&](auto c) -> int {
        LAUNCH(ctx, "bg_ring_solve", (k_ring_solve6<NT_OF(c)>), dim3(d), dim3(64), 0, sys, pa, g, dr, dc, rowsum, act, W, dErrS, probe, (const int *)nullptr, (const int *)nullptr, lam_arr);
        return 0; });
}
// ---- B2b ----
static int fit_solve(RingFit &f) {
    cnmfe_ctx *ctx = f.ctx;
    const unsigned char *act = f.first_run ? nullptr : f.dActive.as<unsigned char>();
    const int probe = (int)ctx->opt("solve_probe", 0);
    if (f.packed) return fit_solve_packed(f, act, probe);
    RET(fit_win_codes(f));
    CovTab tab = f.covtab(); tab.wcodes = ctx->wcodes.as<int>(); tab.woff = f.reach.woff;
    return solve_launch(ctx, f.P, tab, f.g, ctx->rowsum.as<double>(), act, f.nt, probe, ctx->solve_fill.as<double>());
}

int bg_fit_ring(cnmfe_ctx *ctx, Patch *P, int32_t K, const int64_t *A_colptr, const int32_t *A_rowidx, const float *A_val,
                const float *C, int c_order, int with_projection, float *b0_out, int64_t info[4], int b0_only, double thresh_outlier) {
    RingFit f(ctx, P);
    f.K = K; f.A_colptr = A_colptr; f.A_rowidx = A_rowidx; f.A_val = A_val; f.C = C; f.c_order = c_order; f.b0_only = b0_only; f.thresh_outlier = thresh_outlier; f.T = P->T;
    f.outl = thresh_outlier == thresh_outlier; f.has_a = K > 0 && A_colptr[K] > 0; f.a_empty = K == 0;
    RET(ctx->ring_side_join());                              // (option ring_side: the last fit's side work reads the W this fit will write)
    if (f.outl && !P->sn_ready && !(b0_only & 1)) return fail(CNMFE_ESTATE, "fit_ring_model with thresh_outlier needs the noise levels of the block (cnmfe_set_noise)");
    RET(fit_traces_up(f));
    f.ht.mark("traces");
    if (b0_only & 1) {
        RET(fit_upload_csr(f));                               // bg_ssub > 1: b0 = mean(Y - A*C, 2) on the patch (update_background_parallel.m:222-223)
        // (no drain: every upload above went through the pinned arena -- or, too large for it, waited itself -- and what reads b0 is stream-ordered behind this)
        RET(fit_b0(f, bg_geom(P)));
        P->residual.invalidate();
        return 0;
    }
    RET(fit_geometry(f, with_projection));
    fit_lists(f);
    // the window projection first when the video's table exists (a later fit of a patch): the host builds the CSR rows of A, ind_active and the pair tables underneath it
    // (option fit_side: and that set-up is queued on the side stream, so the GPU runs it underneath the projection as well)
    if (f.incr && f.has_a && !f.build_base) RET(fit_queue_projection(f, fit_side_mode(f)));
    f.ht.mark("projection queued");
    if (!f.setup_done) {
        RET(fit_upload_csr(f));
        f.ht.mark("A csr");
        RET(fit_active_b0(f));
        f.ht.mark("ind_active + b0");
    }
    RET(fit_pair_tables(f));
    if (!f.incr || f.build_base) RET(fit_base_table(f));
    if (f.nt < 1 || f.nt > 8) return fail(CNMFE_EUNSUPPORTED, "fit_ring_model: %d ring neighbours (<= %d supported)", P->p, PMAX_RING);
    RET(fit_pack(f));
    if (f.incr) RET(fit_corrections(f, C, c_order));
    f.ht.mark("base / correction launches");
    RET(fit_solve(f));
    // option ring_side: W is final behind this point -- what the NEXT fit asks of it (ring_stats_enqueue) and the W*A tables of the residual request that follows
    // this fit wait for THIS event on the side stream, not for what the compute stream is given after it (resid.hip, ring_side_ahead).  Not the outlier branch, not
    // with lanes, one patch per context
    bool solve_marked = false;
    { const int64_t m = ctx->opt("ring_side", 1);
      if ((m == 1 || m == 2) && !f.outl && ctx->lanes.empty() && ctx->patches.size() == 1) {
          int *dErrAhead = nullptr;
          RET(ctx_errflag(ctx, &dErrAhead));                  // (allocated and cleared in front of the event: the side stream's k_ring_wa may raise it)
          RET(ctx_side_stream(ctx));
          CK(hipEventRecord(ctx->ev_ring_solved, ctx->st()));
          solve_marked = true;
          // (the tables only where a request can be a recorded one at all: residual_plan.hpp -- r1_delta = 0 or r1_lazy = 0 sweep or fold at once, and such a
          //  request builds its own)
          const rplan::ResidualOpts ro = residual_opts(ctx);
          const bool tables = f.has_a && !P->derived && ro.delta != 0 && ro.lazy != 0;
          RET(ring_side_ahead(ctx, P, f.K, tables ? &f.csr : nullptr, A_colptr, A_rowidx, A_val, m == 2));
      } }
    if (!solve_marked) RET(ring_stats_enqueue(ctx, P));                         // what the NEXT fit of this patch asks of the W being written now
    f.ht.mark("solve launch");
    if (b0_out) {
        std::vector<double> tmp(P->d);
        CK(hipMemcpyAsync(tmp.data(), P->b0.p, P->d * sizeof(double), hipMemcpyDeviceToHost, ctx->st()));
        CK(hipStreamSynchronize(ctx->st()));
        for (int64_t i = 0; i < P->d; ++i) b0_out[i] = (float)tmp[i];
        if (f.nactive < 0) f.nactive = *reinterpret_cast<const int *>((const char *)P->stat_host + 8);
    }
    // without b0_out the call returns with the fit in flight (every later engine call is stream-ordered behind it)
    if (info) { info[0] = f.first_run ? 1 : 0; info[1] = f.kstride; info[2] = f.nactive; info[3] = f.pmax; }
    P->residual.invalidate();
    P->residual.solve_marked = solve_marked;
    return 0;
}

// the window projection of ALL frames on the int8 pipe out of a patch's resident digit planes, for callers outside this file (vproj.hip: the spatial update's table):
// digits of the centred traces dCc (K rows, ldc apart), the (block, trace-group pair) items of the lists lst_ptr / blall, one launch; Ut[seg * ut_stride + ...] as
// k_win_proj_i8 leaves it (per-segment partial sums in real units)
int win_i8_table(cnmfe_ctx *ctx, Patch *P, const char *name_dig, const char *name_proj, int K, const float *dCc, int64_t ldc, const std::vector<int> &lst_ptr, const std::vector<int> &blall,
                 const int *dLp, const int *dLk, int nsg, double *dUt, int64_t ut_stride) {
    RET(trace_digits(ctx, name_dig, dCc, ldc, K, P->T, P->dig_T16, false));
    return win_proj_i8_launch(ctx, P, name_proj, lst_ptr, blall, dLp, dLk, nsg, dUt, ut_stride);
}

// loads this translation unit's code object now (HIP loads it at the first launch of one of its kernels -- milliseconds each that would otherwise fall into the first iteration): cnmfe_create
int tu_warm_bg() { hipFuncAttributes at; return hipFuncGetAttributes(&at, (const void *)k_rowsum) == hipSuccess ? 0 : -1; }

}  // namespace cnmfe
