// box_locate_core.h -- which regions a query BOX meets: the classification of one (box, region) pair, shared by locate_box_kernel
// (scene_kernels.h, launched by gcsadmm_scene_locate_boxes of polytope_lp.hip) and its host build (tests/hostemu/locate_box_emu.cpp;
// the product path is the kernel).  The count and fill passes, the ballot and the scan are those of point_locate_core.h.
//
// A start or goal SET of a query is the box [lo, hi], connected to region r iff box and region share a point: one pair LP, decided on
// r* >= -tol.  With the centre c = (lo + hi) / 2 and the half-widths h = (hi - lo) / 2, for row i of the region, a_i x <= b_i:
//
//     g_i = a_i . c - b_i        w_i = sum_k |a_ik| (h_k + 2 tol)        r_i = 2^-40 (sum_k |a_ik c_k| + |b_i|)
//
//   OUT        some row has g_i > w_i + r_i.  Every x of the box widened by tol (infinity norm) then has
//              a_i x - b_i >= g_i - sum_k |a_ik| (h_k + tol) > tol sum_k |a_ik| >= tol |a_i|_2, so the pair LP's r* is below -tol:
//              the argument of point_locate_core.h with eps replaced per axis by h_k;
//   IN         every row has g_i <= -r_i: the centre itself lies in the region;
//   UNDECIDED  otherwise.  A box as wide as a region leaves many pairs here -- every region that reaches into the box without holding
//              its centre -- and these alone go to the pair LP.
//
// g_i and the sum of r_i are one fma chain each in index order, and w_i + r_i is one more chain that starts from r_i, so no product is
// left for the compiler to contract or not: the host build and the kernel classify bit for bit alike.  c_k and h_k + 2 tol are formed
// once on the host (locate_box_prepare) and both read the same doubles.
#pragma once
#include "point_locate_core.h"

namespace gcsadmm_lp {

// the box as the classifier reads it: out[0 .. n) = c, out[n .. 2n) = h + 2 tol
inline void locate_box_prepare(int n, const double *lo, const double *hi, double tol, double *out)
{
    for (int k = 0; k < n; ++k) {
        out[k] = 0.5 * lo[k] + 0.5 * hi[k];
        out[n + k] = (0.5 * hi[k] - 0.5 * lo[k]) + 2.0 * tol;
    }
}

// c[N], hw[N] = h + 2 tol
template <int N> GCS_LOCATE_HD int locate_box_classify(const LocateRegions &R, int region, const double *c, const double *hw)
{
    const int first = R.ptr[region], last = R.ptr[region + 1];
    bool in = true;
    for (int i = first; i < last; ++i) {
        const double *a = R.A + (size_t)i * N;
        const double bi = R.b[i];
        double g = -bi, mag = fabs(bi);
#pragma unroll
        for (int k = 0; k < N; ++k) {
            g = fma(a[k], c[k], g);
            mag = fma(fabs(a[k]), fabs(c[k]), mag);
        }
        const double r = 0x1p-40 * mag;
        double w = r;
#pragma unroll
        for (int k = 0; k < N; ++k) w = fma(fabs(a[k]), hw[k], w);
        if (g > w) return LOCATE_OUT;
        in = in && g <= -r;
    }
    return in ? LOCATE_IN : LOCATE_UNDECIDED;
}

// the class of a lane's region (OUT past the end)
template <int N> GCS_LOCATE_HD int locate_box_lane(const LocateRegions &R, int region, const double *c, const double *hw)
{
    return region >= 0 ? locate_box_classify<N>(R, region, c, hw) : LOCATE_OUT;
}

} // namespace gcsadmm_lp
