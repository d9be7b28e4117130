// Image operations on single footprints: one workgroup per neuron, the neuron's box in LDS (the family k_connectivity started; included by factor.hip).
//
//   k_fp_circular           endoscope/circular_constraints.m:8-55                                          (Sources2D.compactSpatial, spatial_constraints.circular)
//   k_fp_threshold_dilate   utilities/threshold_components.m:20-62 + determine_search_location.m:89-98     (search_method = 'dilate')
//   k_fp_trim               @Sources2D/Sources2D.m:942-965                                                  (Sources2D.trimSpatial)
//
// Rules all three keep (include/cnmfe.h, "footprint image operations"):
//   * a box is a rectangle of the field of view, column-major like the image, at most FP_MAX_CELLS cells; a cell outside the box but inside the field of
//     view is a zero of the image (the host sizes the box so that this is true), a cell outside the field of view follows the padding rule of the operation
//   * every decision -- a comparison, a selection, a sum somebody compares -- is taken in fp64 on the fp32 values of A, with __dmul_rn / __dadd_rn /
//     __dsub_rn: no contraction into an fma, the roundings of the NumPy statement in cnmf_e_amd/hostops.py, in its order
//   * every loop that iterates to a fixed point is bounded by the number of cells of the box
//   * plain vector stores, no atomics, one order of evaluation: two calls give the same bits
#pragma once
// (included inside namespace cnmfe)

constexpr int FP_NT = 256;              // threads of a workgroup
constexpr int FP_MAX_CELLS = 4096;      // cells of the largest box (Engine.IMAGE_OPS_MAX_BOX); LDS of k_fp_threshold_dilate: 2 x 16 KB images + 32 KB sort keys + 8 KB
                                        // bitmaps + 3 KB reductions = 77 KB of the CU's 160 KB: two workgroups per CU
constexpr int FP_MAX_SE = 15;           // largest side of the structuring element of the dilation (reach 7: strel('disk', 7, 0))
constexpr int FP_CLOSE_MARGIN = 2;      // cells the 3 x 3 median (1) and the closing at a border of the field of view (1 more) can reach beyond the non-zeros

struct FpGeom { int r0, c0, h, w, n, d1, d2; };

__device__ inline FpGeom fp_geom(const int4 bx, int d1, int d2) { return FpGeom{bx.x, bx.y, bx.z, bx.w, bx.z * bx.w, d1, d2}; }
__device__ inline bool fp_in_box(const FpGeom &g, int lr, int lc) { return lr >= 0 && lr < g.h && lc >= 0 && lc < g.w; }
__device__ inline bool fp_in_fov(const FpGeom &g, int lr, int lc) { return g.r0 + lr >= 0 && g.r0 + lr < g.d1 && g.c0 + lc >= 0 && g.c0 + lc < g.d2; }

// box load from CSC: img[lc * h + lr]; an entry outside the box (a stored zero: the box spans the non-zeros) is skipped.  Ends with a barrier.
__device__ inline void fp_load_box(const int64_t *__restrict__ colptr, const int *__restrict__ erow, const float *__restrict__ aval, int k, const FpGeom &g, float *img) {
    for (int i = threadIdx.x; i < g.n; i += FP_NT) img[i] = 0.f;
    __syncthreads();
    const int64_t e0 = colptr[k], e1 = colptr[k + 1];
    for (int64_t e = e0 + threadIdx.x; e < e1; e += FP_NT) {
        const int pix = erow[e], lr = pix % g.d1 - g.r0, lc = pix / g.d1 - g.c0;
        if (fp_in_box(g, lr, lc)) img[lc * g.h + lr] = aval[e];
    }
    __syncthreads();
}

// medfilt2(img, [3 3]) at one cell: the fifth of the nine values, zeros outside the box (medfilt2 pads with zeros; beyond the box the image is zero)
__device__ inline float fp_median9(const float *img, const FpGeom &g, int lr, int lc) {
    float v[9];
#pragma unroll
    for (int j = 0; j < 9; ++j) {
        const int rr = lr + j % 3 - 1, cc = lc + j / 3 - 1;
        v[j] = fp_in_box(g, rr, cc) ? img[cc * g.h + rr] : 0.f;
    }
#pragma unroll
    for (int a = 1; a < 9; ++a)
#pragma unroll
        for (int b = a; b > 0; --b) {
            const float lo = v[b - 1], hi = v[b];
            const bool sw = hi < lo;
            v[b - 1] = sw ? hi : lo; v[b] = sw ? lo : hi;
        }
    return v[4];
}

// binary 3 x 3 dilation / erosion at one cell.  Dilation: false outside the box.  Erosion: true outside the field of view (imerode pads with +Inf), false
// outside the box inside it.
__device__ inline unsigned char fp_dilate3(const unsigned char *bw, const FpGeom &g, int lr, int lc) {
    unsigned char any = 0;
    for (int dc = -1; dc <= 1; ++dc) for (int dr = -1; dr <= 1; ++dr)
        if (fp_in_box(g, lr + dr, lc + dc)) any |= bw[(lc + dc) * g.h + lr + dr];
    return any;
}
__device__ inline unsigned char fp_erode3(const unsigned char *bw, const FpGeom &g, int lr, int lc) {
    unsigned char all = 1;
    for (int dc = -1; dc <= 1; ++dc) for (int dr = -1; dr <= 1; ++dr) {
        if (fp_in_box(g, lr + dr, lc + dc)) all &= bw[(lc + dc) * g.h + lr + dr];
        else if (fp_in_fov(g, lr + dr, lc + dc)) all = 0;
    }
    return all;
}

// grey erosion / dilation by a (2 half + 1)^2 square at one cell of a non-negative image: cells outside the field of view are left out (+Inf / -Inf padding),
// cells outside the box inside it count as zero
__device__ inline float fp_grey_erode(const float *img, const FpGeom &g, int lr, int lc, int half) {
    float m = INFINITY;
    for (int dc = -half; dc <= half; ++dc) for (int dr = -half; dr <= half; ++dr) {
        if (!fp_in_fov(g, lr + dr, lc + dc)) continue;
        m = fminf(m, fp_in_box(g, lr + dr, lc + dc) ? img[(lc + dc) * g.h + lr + dr] : 0.f);
    }
    return m;
}
__device__ inline float fp_grey_dilate(const float *img, const FpGeom &g, int lr, int lc, int half) {
    float m = -INFINITY;
    for (int dc = -half; dc <= half; ++dc) for (int dr = -half; dr <= half; ++dr) {
        if (!fp_in_fov(g, lr + dr, lc + dc)) continue;
        m = fmaxf(m, fp_in_box(g, lr + dr, lc + dc) ? img[(lc + dc) * g.h + lr + dr] : 0.f);
    }
    return m;
}

// 4- or 8-connected components by min-label propagation: lab holds 0 (background) or a positive id that is unique per cell; afterwards every cell of a component
// holds the smallest id of the component.  A sweep lowers at least one label or is the last: at most n sweeps (the longest path inside a box of n cells).
// In-place reads may see a neighbour's old or new label; both belong to the component and labels only fall, so the fixed point -- the result -- is the same.
__device__ inline void fp_label(int *lab, const FpGeom &g, bool eight, int *changed) {
    for (int iter = 0; iter < g.n; ++iter) {
        if (threadIdx.x == 0) *changed = 0;
        __syncthreads();
        for (int i = threadIdx.x; i < g.n; i += FP_NT) {
            const int l = lab[i];
            if (!l) continue;
            const int lr = i % g.h, lc = i / g.h;
            int best = l;
            for (int dc = -1; dc <= 1; ++dc) for (int dr = -1; dr <= 1; ++dr) {
                if ((!dr && !dc) || (!eight && dr && dc) || !fp_in_box(g, lr + dr, lc + dc)) continue;
                const int v = lab[(lc + dc) * g.h + lr + dr];
                if (v && v < best) best = v;
            }
            if (best < l) { lab[i] = best; *changed = 1; }
        }
        __syncthreads();
        if (!*changed) break;
        __syncthreads();
    }
    __syncthreads();
}

// the largest v of the workgroup, among equals the smallest i: into redv[0], redi[0].  Ends with a barrier.
__device__ inline void fp_argbest(double v, int i, double *redv, int *redi) {
    redv[threadIdx.x] = v; redi[threadIdx.x] = i;
    __syncthreads();
    for (int o = FP_NT / 2; o > 0; o >>= 1) {
        if ((int)threadIdx.x < o) {
            const double v2 = redv[threadIdx.x + o]; const int i2 = redi[threadIdx.x + o];
            if (v2 > redv[threadIdx.x] || (v2 == redv[threadIdx.x] && i2 < redi[threadIdx.x])) { redv[threadIdx.x] = v2; redi[threadIdx.x] = i2; }
        }
        __syncthreads();
    }
}
// the first maximum of img in column-major order (the zeros of the box count)
__device__ inline void fp_argmax_box(const float *img, const FpGeom &g, double *redv, int *redi) {
    double bv = -INFINITY; int bi = 0x7fffffff;
    for (int i = threadIdx.x; i < g.n; i += FP_NT) { const double v = img[i]; if (v > bv) { bv = v; bi = i; } }   // (ascending i per thread: the first of equals stays)
    fp_argbest(bv, bi, redv, redi);
}

// ---- (a) circular_constraints.m:8-55 on the bounding box of the non-zeros (the reference recurses on the crop: its edges are the image's) ----------------------
// box[k] = (r0, c0, h, w) of the non-zeros, h = 0: nothing to do (an empty column, or one the host computes).  out + off[k]: the new column's values over the box.
__global__ void __launch_bounds__(FP_NT) k_fp_circular(const int64_t *__restrict__ colptr, const int *__restrict__ erow, const float *__restrict__ aval,
                                                       const int4 *__restrict__ box, const int64_t *__restrict__ off, int d1, int d2, float *__restrict__ out) {
    __shared__ float sub[FP_MAX_CELLS];
    __shared__ float cut[FP_MAX_CELLS];
    __shared__ int lab[FP_MAX_CELLS];
    __shared__ unsigned char bw[FP_MAX_CELLS];
    __shared__ double redv[FP_NT]; __shared__ int redi[FP_NT]; __shared__ int changed;
    const int k = blockIdx.x;
    const FpGeom g = fp_geom(box[k], d1, d2);
    if (g.n <= 0 || g.n > FP_MAX_CELLS) return;
    float *o = out + off[k];
    fp_load_box(colptr, erow, aval, k, g, sub);
    if (g.h < 2 || g.w < 2) {                                                                       // :17-19: returned as it is
        for (int i = threadIdx.x; i < g.n; i += FP_NT) o[i] = sub[i];
        return;
    }
    fp_argmax_box(sub, g, redv, redi);                                                              // :30
    const int imax = redi[0] < g.n ? redi[0] : 0, y0 = imax % g.h, x0 = imax / g.h;
    const double third = redv[0] / 3.0;
    __syncthreads();
    for (int i = threadIdx.x; i < g.n; i += FP_NT) {
        const int lr = i % g.h, lc = i / g.h;
        const float v = sub[i];
        // gradient(): central differences, one-sided at the edges of the crop (:33)
        const double fy = lr == 0 ? __dsub_rn((double)sub[i + 1], (double)v) : lr == g.h - 1 ? __dsub_rn((double)v, (double)sub[i - 1])
                                  : __dmul_rn(__dsub_rn((double)sub[i + 1], (double)sub[i - 1]), 0.5);
        const double fx = lc == 0 ? __dsub_rn((double)sub[i + g.h], (double)v) : lc == g.w - 1 ? __dsub_rn((double)v, (double)sub[i - g.h])
                                  : __dmul_rn(__dsub_rn((double)sub[i + g.h], (double)sub[i - g.h]), 0.5);
        const double s = __dadd_rn(__dmul_rn(fx, (double)(x0 - lc)), __dmul_rn(fy, (double)(y0 - lr)));
        const float c = (s < 0.0 && (double)v < third) ? 0.f : v;                                    // :34-35
        cut[i] = c;
        lab[i] = c != 0.f ? i + 1 : 0;
    }
    __syncthreads();
    fp_label(lab, g, false, &changed);                                                              // :39 bwlabel(., 4)
    const int lpeak = lab[imax];
    for (int i = threadIdx.x; i < g.n; i += FP_NT) bw[i] = lab[i] == lpeak;
    __syncthreads();
    for (int i = threadIdx.x; i < g.n; i += FP_NT) sub[i] = fp_dilate3(bw, g, i % g.h, i / g.h) ? cut[i] : 0.f;   // :40-41
    __syncthreads();
    for (int i = threadIdx.x; i < g.n; i += FP_NT) o[i] = fp_median9(sub, g, i % g.h, i / g.h);                  // :42
}

// ---- (b) threshold_components.m:20-62 + imdilate (determine_search_location.m:89-98) --------------------------------------------------------------------
// box[k]: the non-zeros grown by FP_CLOSE_MARGIN + the reach of se, clipped to the field of view.  plain != 0: one of the last nb columns, dilated from > 0 (:22,25).
// se: sh x sw bytes, row-major, odd sides, origin at the centre.  out + off[k]: one byte per cell of the box, 1 = in the index set.
__global__ void __launch_bounds__(FP_NT) k_fp_threshold_dilate(const int64_t *__restrict__ colptr, const int *__restrict__ erow, const float *__restrict__ aval,
                                                               const int4 *__restrict__ box, const int64_t *__restrict__ off, int d1, int d2, int K, int nb, double frac,
                                                               const unsigned char *__restrict__ se, int sh, int sw, unsigned char *__restrict__ out) {
    __shared__ float raw[FP_MAX_CELLS];
    __shared__ float img[FP_MAX_CELLS];                          // the median-filtered image
    __shared__ unsigned long long keys[FP_MAX_CELLS];            // the sort; afterwards the labels
    __shared__ unsigned char bw[FP_MAX_CELLS];
    __shared__ unsigned char bw2[FP_MAX_CELLS];
    __shared__ unsigned char sse[FP_MAX_SE * FP_MAX_SE];
    __shared__ double redv[FP_NT]; __shared__ int redi[FP_NT]; __shared__ int changed; __shared__ int first;
    int *lab = reinterpret_cast<int *>(keys);
    const int k = blockIdx.x;
    const FpGeom g = fp_geom(box[k], d1, d2);
    if (g.n <= 0 || g.n > FP_MAX_CELLS || sh > FP_MAX_SE || sw > FP_MAX_SE) return;
    unsigned char *o = out + off[k];
    for (int i = threadIdx.x; i < sh * sw; i += FP_NT) sse[i] = se[i];
    fp_load_box(colptr, erow, aval, k, g, raw);
    if (k >= K - nb) {
        for (int i = threadIdx.x; i < g.n; i += FP_NT) bw2[i] = raw[i] > 0.f;
        __syncthreads();
    } else {
        for (int i = threadIdx.x; i < g.n; i += FP_NT) img[i] = fp_median9(raw, g, i % g.h, i / g.h);              // :28
        __syncthreads();
        // sort ascending by (e = a^2, column-major index) (:31, MATLAB's sort is stable).  a is fp32: a^2 is exact in fp64 and ordered like |a|, whose bits order like
        // its value -- the key is (bits of |a|, index).  Bitonic network over the next power of two, padded with the largest key.
        int np2 = 1; while (np2 < g.n) np2 <<= 1;
        for (int i = threadIdx.x; i < np2; i += FP_NT)
            keys[i] = i < g.n ? ((unsigned long long)__float_as_uint(fabsf(img[i])) << 32) | (unsigned)i : ~0ull;
        __syncthreads();
        for (int k2 = 2; k2 <= np2; k2 <<= 1)
            for (int j = k2 >> 1; j > 0; j >>= 1) {
                for (int i = threadIdx.x; i < np2; i += FP_NT) {
                    const int p = i ^ j;
                    if (p > i) {
                        const unsigned long long a = keys[i], b = keys[p];
                        if ((a > b) == ((i & k2) == 0)) { keys[i] = b; keys[p] = a; }
                    }
                }
                __syncthreads();
            }
        // the SEQUENTIAL cumulative sum in that order (:32), by one lane: the total, then the first place above (1 - nrgthr) * total (:33)
        if (threadIdx.x == 0) {
            double total = 0.0;
            for (int j = 0; j < g.n; ++j) { const double a = img[(int)(keys[j] & 0xffffffffu)]; total = __dadd_rn(total, __dmul_rn(a, a)); }
            const double bound = __dmul_rn(frac, total);
            double cs = 0.0; int f = g.n;
            for (int j = 0; j < g.n; ++j) {
                const double a = img[(int)(keys[j] & 0xffffffffu)]; cs = __dadd_rn(cs, __dmul_rn(a, a));
                if (cs > bound) { f = j; break; }
            }
            first = f;
        }
        for (int i = threadIdx.x; i < g.n; i += FP_NT) bw[i] = 0;
        __syncthreads();
        for (int j = first + threadIdx.x; j < g.n; j += FP_NT) bw[(int)(keys[j] & 0xffffffffu)] = 1;                 // :35
        __syncthreads();
        // imclose by the 3 x 3 square (:37)
        for (int i = threadIdx.x; i < g.n; i += FP_NT) bw2[i] = fp_dilate3(bw, g, i % g.h, i / g.h);
        __syncthreads();
        for (int i = threadIdx.x; i < g.n; i += FP_NT) bw[i] = fp_erode3(bw2, g, i % g.h, i / g.h);
        __syncthreads();
        // 8-connected labels (:39).  The ids count in row-major order like the labels of the host statement, whose first maximum the tie rule below follows.
        for (int i = threadIdx.x; i < g.n; i += FP_NT) lab[i] = bw[i] ? (i % g.h) * g.w + i / g.h + 1 : 0;
        __syncthreads();
        fp_label(lab, g, true, &changed);
        // the component with the most energy of the FILTERED image (:43-47): fp64, summed in row-major order
        double bv = -INFINITY; int bl = 0x7fffffff;
        for (int i = threadIdx.x; i < g.n; i += FP_NT) {
            const int id = (i % g.h) * g.w + i / g.h + 1;
            if (lab[i] != id) continue;                                                                // (i is the first cell of its component)
            double s = 0.0;
            for (int r = 0; r < g.h; ++r) for (int c = 0; c < g.w; ++c)
                if (lab[c * g.h + r] == id) { const double a = img[c * g.h + r]; s = __dadd_rn(s, __dmul_rn(a, a)); }
            if (s > bv || (s == bv && id < bl)) { bv = s; bl = id; }
        }
        fp_argbest(bv, bl, redv, redi);
        const int lbest = redi[0] == 0x7fffffff ? -1 : redi[0];
        // Ath holds the filtered values on that component; the dilation starts from Ath > 0 (determine_search_location.m:92)
        for (int i = threadIdx.x; i < g.n; i += FP_NT) bw2[i] = lab[i] == lbest && img[i] > 0.f;
        __syncthreads();
    }
    // imdilate by se, clipped at the field of view (:92-93)
    const int ch = sh / 2, cw = sw / 2;
    for (int i = threadIdx.x; i < g.n; i += FP_NT) {
        const int lr = i % g.h, lc = i / g.h;
        unsigned char any = 0;
        for (int a = 0; a < sh && !any; ++a) for (int b = 0; b < sw; ++b) {
            if (!sse[a * sw + b]) continue;
            const int rr = lr - (a - ch), cc = lc - (b - cw);
            if (fp_in_box(g, rr, cc) && bw2[cc * g.h + rr]) { any = 1; break; }
        }
        o[i] = any;
    }
}

// ---- (c) Sources2D.m:942-965 (trimSpatial) on the bounding box of the non-zeros of a non-negative footprint -----------------------------------------------
// The opening is below the image, so everything above the threshold lies inside the box; keep[e] = 1 where l == l(ind_max); cnt[k] = sum(ai > 0) afterwards.
__global__ void __launch_bounds__(FP_NT) k_fp_trim(const int64_t *__restrict__ colptr, const int *__restrict__ erow, const float *__restrict__ aval,
                                                   const int4 *__restrict__ box, int d1, int d2, double thr, int half, unsigned char *__restrict__ keep, int *__restrict__ cnt) {
    __shared__ float img[FP_MAX_CELLS];
    __shared__ float er[FP_MAX_CELLS];
    __shared__ int lab[FP_MAX_CELLS];
    __shared__ double redv[FP_NT]; __shared__ int redi[FP_NT]; __shared__ int changed;
    const int k = blockIdx.x;
    const FpGeom g = fp_geom(box[k], d1, d2);
    if (g.n <= 0 || g.n > FP_MAX_CELLS) return;
    fp_load_box(colptr, erow, aval, k, g, img);
    fp_argmax_box(img, g, redv, redi);
    const double vmax = ((int64_t)g.n < (int64_t)d1 * d2) ? fmax(redv[0], 0.0) : redv[0];              // max(ai) sees the zeros outside the box
    __syncthreads();
    for (int i = threadIdx.x; i < g.n; i += FP_NT) er[i] = fp_grey_erode(img, g, i % g.h, i / g.h, half);
    __syncthreads();
    const double bound = __dmul_rn(vmax, thr);
    for (int i = threadIdx.x; i < g.n; i += FP_NT) {                                                  // ai_open, temp = ai_open > max(ai) * thr (:951-953)
        const float op = fp_grey_dilate(er, g, i % g.h, i / g.h, half);
        img[i] = op;
        lab[i] = (double)op > bound ? i + 1 : 0;
    }
    __syncthreads();
    fp_argmax_box(img, g, redv, redi);                                                               // :955 (over the opened image)
    const int imax = redi[0] < g.n ? redi[0] : 0;
    fp_label(lab, g, false, &changed);                                                               // :954
    const int lmax = lab[imax];
    int c = 0;
    const int64_t e0 = colptr[k], e1 = colptr[k + 1];
    for (int64_t e = e0 + threadIdx.x; e < e1; e += FP_NT) {
        const int pix = erow[e], lr = pix % d1 - g.r0, lc = pix / d1 - g.c0;
        const bool kp = !fp_in_box(g, lr, lc) || lab[lc * g.h + lr] == lmax;                          // :957
        keep[e] = kp;
        c += kp && aval[e] > 0.f;
    }
    __syncthreads();
    redi[threadIdx.x] = c;
    __syncthreads();
    for (int o = FP_NT / 2; o > 0; o >>= 1) { if ((int)threadIdx.x < o) redi[threadIdx.x] += redi[threadIdx.x + o]; __syncthreads(); }
    if (threadIdx.x == 0) cnt[k] = redi[0];                                                          // :958
}

