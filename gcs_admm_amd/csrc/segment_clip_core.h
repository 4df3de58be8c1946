// segment_clip_core.h -- through which regions a segment runs, and whether they cover it: the span of one (segment, region) pair, the
// pieces of the count and fill passes of segment_clip_kernel, and the steps of the cover test of segment_chain_kernel (scene_kernels.h),
// shared with their host build (tests/hostemu/clip_emu.cpp; the product path is the kernels).
//
// The span.  Segment q is x(t) = p + t d, t in [0, 1], with d_k = q_k - p_k rounded once; from then on d is data.  For row i of the
// region, a_i x <= b_i:
//
//     g = fma chain from -b_i over a_ik p_k               h = fma chain from 0 over a_ik d_k
//     mag = fma chain from |b_i| over |a_ik||p_k|, |a_ik||d_k| (both per k, in this order)       s = sum_k |a_ik| (adds in index order)
//     m = fma(tol, s, 2^-40 mag)                          c = m - g
//     h > 0: t_out = min(t_out, c / h)     h < 0: t_in = max(t_in, c / h)     h == 0 and c < 0: no span
//
// from [t_in, t_out] = [0, 1]; the pair is a hit iff t_in <= t_out at the end, of class WHOLE (t_in == 0 and t_out == 1) or PART.
// min and max are written as comparisons (a bound replaces the kept one only when it is strictly tighter), so a -0.0 quotient never
// replaces t_in = +0.0.  Only the written fma calls fuse: no other product stands next to a sum.
//
// The contract (the sandwich).  With S = sum_k |a_ik| and MAG = |b_i| + sum_k |a_ik| (|p_k| + |d_k|) exact, every span
//     contains  the exact span of the region with every row relaxed to a_i x <= b_i + tol S, and
//     lies in   the exact span of the region with every row relaxed to a_i x <= b_i + tol S (1 + 2^-40) + 2^-39 MAG.
// (tol S >= tol |a_i|_2: the convention of locate_classify; the rest is the allowance for the rounding of the rule itself.)
//
// Derivation, u = 2^-53, gamma_k = k u / (1 - k u), no overflow or underflow.  Write G = a_i.p - b_i and H = a_i.d.  For t in [0, 1]
// the three branches are one statement: the row admits t iff t h <= c (1 + d2), d2 the rounding of the division (h = 0: c >= 0), and
// with c = (m - g)(1 + d1) that is  g + t h <= m + z,  |z| <= gamma_2 (m + |g|).
//   * g + t h = G + t H + x with |x| <= gamma_n MAG (two fma chains of n steps; t <= 1).
//   * s = S (1 + e_s), |e_s| <= gamma_(n-1); mag = MAG (1 + e_m), |e_m| <= gamma_2n; 2^-40 mag is exact, m rounds once.
//   Case tol S > 2 MAG.  |G| + |H| <= MAG, so G + t H - tol S < -MAG < 0 for every t in [0, 1]: the exact row, relaxed by tol S or by
//   more, admits all of [0, 1].  So does the computed one: m >= tol S (1 - gamma_n) > 1.9 MAG and |g| + |h| <= (1 + gamma_n) MAG give
//   c > |h|, hence c / h > 1 (h > 0), < 0 (h < 0), and c > 0 (h = 0).  The row changes neither span.
//   Case tol S <= 2 MAG.  Every error is a multiple of u MAG: m = tol S + 2^-40 MAG + y with |y| <= (2 gamma_n + 2^-39 gamma_2n + 3 u) MAG,
//   m + |g| <= 3.01 MAG so |z| <= 7 u MAG, and altogether the row admits t iff
//       G + t H <= tol S + 2^-40 MAG + w,     |w| <= (3 n + 12) u MAG <= 36 u MAG < 2^-47 MAG      (n <= 8).
//   2^-40 MAG - |w| > 0: every t the row relaxed by tol S admits is admitted.  2^-40 MAG + |w| < 2^-39 MAG: every admitted t satisfies
//   the row relaxed by tol S + 2^-39 MAG.  (The factor 1 + 2^-40 of the outer relaxation is not needed; it is kept as stated.)
// The intersection over the rows and with [0, 1] keeps both inclusions.  The constant 2^-40 is that of locate_classify; the derivation
// needs only that it exceeds 36 u = 2^-47.8.
//
// The list has the shape of locate_kernel (point_locate_core.h): one 64-lane workgroup per (chunk of LOCATE_CHUNK regions, segment),
// one region per lane, a count pass and a fill pass, ballot + prefix count, the host scan locate_scan.  No atomics; ordered by segment,
// then region index; the same on every run.  The fill pass stores t_in and t_out of every hit beside its region and class.
//
// The chain (cover test) of a segment: a greedy sweep over its hits from cur = 0.  While cur < 1: among the hits with
// t_in <= cur < t_out take the one of largest t_out, the first in the list among equals; append it and set cur = t_out.  No such hit:
// GAP at reach = cur.  Otherwise COVERED, and reach == 1.0 exactly (no t_out exceeds 1).  cur grows strictly and a hit taken once
// never qualifies again, so the chain is at most as long as the segment's list: it is written at the segment's own offset.  One
// 64-lane wavefront per segment: each step is a lane-local best over the hits lane, lane + 64, ... (chain_lane_best) and one wave
// reduction on (t_out, list position) (chain_better is its total order).  Only comparisons: host and device agree bit for bit.
#pragma once
#include "point_locate_core.h"

namespace gcsadmm_lp {

constexpr int CLIP_OUT = 0, CLIP_WHOLE = 1, CLIP_PART = 2;
constexpr int COVER_COVERED = 0, COVER_GAP = 1;
constexpr int CHAIN_NONE = 0x7fffffff;      // "no hit qualifies": above every position of a segment's list

// d = q - p, rounded once
template <int N> GCS_LOCATE_HD void clip_direction(const double *p, const double *q, double *d)
{
#pragma unroll
    for (int k = 0; k < N; ++k) d[k] = q[k] - p[k];
}

// the span of (segment p + t d, region): the class, and for a hit t_in, t_out
template <int N> GCS_LOCATE_HD int clip_span(const LocateRegions &R, int region, const double *p, const double *d, double tol, double *t_in, double *t_out)
{
    const int first = R.ptr[region], last = R.ptr[region + 1];
    double lo = 0.0, hi = 1.0;
    for (int i = first; i < last; ++i) {
        const double *a = R.A + (size_t)i * N;
        const double bi = R.b[i];
        double g = -bi, h = 0.0, mag = fabs(bi), s = 0.0;
#pragma unroll
        for (int k = 0; k < N; ++k) {
            g = fma(a[k], p[k], g);
            h = fma(a[k], d[k], h);
            mag = fma(fabs(a[k]), fabs(p[k]), mag);
            mag = fma(fabs(a[k]), fabs(d[k]), mag);
            s += fabs(a[k]);
        }
        const double m = fma(tol, s, 0x1p-40 * mag);
        const double c = m - g;
        if (h > 0.0) {
            const double t = c / h;
            if (t < hi) hi = t;
        } else if (h < 0.0) {
            const double t = c / h;
            if (t > lo) lo = t;
        } else if (c < 0.0) {
            return CLIP_OUT;
        }
        if (!(lo <= hi)) return CLIP_OUT;      // (the bounds only tighten: no later row brings the span back)
    }
    *t_in = lo; *t_out = hi;
    return lo == 0.0 && hi == 1.0 ? CLIP_WHOLE : CLIP_PART;
}

// one lane's part of one stride (locate_region has its region): the class, OUT past the end
template <int N> GCS_LOCATE_HD int clip_lane(const LocateRegions &R, int region, const double *p, const double *d, double tol, double *t_in, double *t_out)
{
    return region >= 0 ? clip_span<N>(R, region, p, d, tol, t_in, t_out) : CLIP_OUT;
}
// ... and its store in the fill pass: locate_store with the span
GCS_LOCATE_HD void clip_store(int *hit_region, unsigned char *hit_class, double *hit_in, double *hit_out, long long pos, long long limit,
                              unsigned long long mask, int lane, int region, int cls, double t_in, double t_out)
{
    if (cls == CLIP_OUT) return;
    const long long at = pos + locate_rank(mask, lane);
    if (at < limit) {
        hit_region[at] = region;
        hit_class[at] = (unsigned char)cls;
        hit_in[at] = t_in;
        hit_out[at] = t_out;
    }
}

// ---- the chain ----
// (t_out, position) a is a better next member than b: the larger t_out, the earlier position among equals.  A total order on distinct
// positions, so a reduction in any order finds the same best
GCS_LOCATE_HD bool chain_better(double a_out, int a_pos, double b_out, int b_pos)
{
    return a_pos != CHAIN_NONE && (b_pos == CHAIN_NONE || a_out > b_out || (a_out == b_out && a_pos < b_pos));
}

// One lane's best among the hits lane, lane + 64, ... of a segment's list of `count` spans at (t_in, t_out): the spans that hold cur.
// (first_in, first_out): the span at position `lane`, which the lane keeps from step to step (the first 64 spans stay in registers).
GCS_LOCATE_HD void chain_lane_best(const double *t_in, const double *t_out, int count, int lane, double first_in, double first_out, double cur,
                                   double *best_out, int *best_pos)
{
    double bo = 0.0;
    int bp = CHAIN_NONE;
    for (int j = lane; j < count; j += LOCATE_WAVE) {
        const double in = j == lane ? first_in : t_in[j], out = j == lane ? first_out : t_out[j];
        if (in <= cur && cur < out && chain_better(out, j, bo, bp)) { bo = out; bp = j; }
    }
    *best_out = bo; *best_pos = bp;
}

} // namespace gcsadmm_lp
