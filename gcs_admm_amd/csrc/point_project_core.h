// point_project_core.h -- the nearest regions of a point that may lie in none: the Euclidean projection of one point onto one region,
// the candidate test in front of it and the pieces of the list and solve passes, shared by project_list_kernel and project_solve_kernel
// (scene_kernels.h, launched by gcsadmm_scene_project_points of polytope_lp.hip) and their host build (tests/hostemu/project_emu.cpp; the
// product path is the kernels).  The count and fill passes, the ballot and the scan are those of point_locate_core.h.
//
// For point p and region r with rows a_i x <= b_i, every row is taken normalised: a^_i = a_i / |a_i|_2, b^_i = b_i / |a_i|_2 (the squares
// summed in ascending coordinate order), so that a row multiplied by any positive factor changes nothing but rounding.
//
//     g_i = a^_i . p - b^_i        m_i = sum_k |a^_ik p_k| + |b^_i|
//
//   lower bound   max(0, max_i g_i): the distance to the most violated half-space, never more than the distance to the region;
//   candidate     unless some row has g_i > radius (1 + 1e-9) + 2^-40 m_i (the margin of locate_classify, widened in the same way:
//                 it lists more pairs and never loses one).  radius is per point and may be +inf.  No boxes, no centres;
//   INSIDE        no row has g_i > 0: class 1, x = p with the same bits, d = 0, no iteration.  Every other candidate is of class 2;
//   projection    x* = argmin 1/2 |x - p|^2 subject to A^ x <= b^ by the dual active-set method of Goldfarb and Idnani with the identity as
//                 Hessian: x = p - N' u, u >= 0 on a working set N of at most n rows that x satisfies with equality.
//                   1. the most violated row j outside the working set, the lowest index among equals; none: done.  A row counts as
//                      violated with g_j > 0 before the first step and with g_j > 2^-44 m_j (at x) afterwards, a sixteenth of the
//                      allowance of locate_classify;
//                   2. z = (I - N'(N N')^-1 N) a^_j and r = (N N')^-1 N a^_j from N = L Q, Q with orthonormal rows (modified
//                      Gram-Schmidt), L lower triangular -- the Cholesky factor of N N', kept as the factor and never squared:
//                      c = Q a^_j and z come out of one more Gram-Schmidt row, r = L^-T c;
//                   3. the primal step t1 = g_j / |z|^2 and the dual step t2 = min u_i / r_i over r_i > 0, the lowest position among
//                      equals; t = min(t1, t2): x -= t z, u -= t r, u_j += t;
//                   4. t2 < t1: the row of t2 leaves the working set, L and Q are rebuilt from the rows that stay and the same row j
//                      is tried again; otherwise row j enters the working set (its row of L and Q is already there);
//                   5. |z|^2 <= 2^-80 (PROJECT_SPAN: the rows have length 1, so |z| is the sine of the angle between row j and the
//                      span of the working set, and below 2^-40 it is what the rounding of n unit vectors leaves of a row in that
//                      span), or a full working set: the dual step alone.  No r_i > 0 then: no step is available.
//                 Every step, primal or dual, counts as one iteration.  At the end one correction dx = Q' L^-1 (N x - b^) puts x on its
//                 working rows up to the rounding of x itself (the steps round relative to |p|): project_polish;
//   distance      d = informed_distance(x, p, n);
//   status        0 solved and d <= radius (a plain compare); 1 solved, beyond the radius (the pair stays in the list); -1 failed: the
//                 iteration limit, a non-finite value, or no step available -- x and d are then the last iterate's, not a projection.
//
// Nothing here is contracted: g_i and m_i are one written fma chain each, everything else is a product or a sum rounded on its own
// (GCS_INFORMED_EXACT_FN / _BODY of informed_core.h), divisions and square roots are plain / and sqrt.  The host build and the
// kernels give the same bits.  The working set of a lane -- x, u, the row indices, L, Q and the directions -- is indexed by constants
// alone after unrolling (the loops have the bound N and are predicated on the size of the working set; a place past the working set
// holds a zero row of Q and a unit row of L, so the sums need no predicate), and the rows come from the polytope CSR by index.
#pragma once
#include "informed_core.h"
#include "point_locate_core.h"

namespace gcsadmm_lp {

constexpr int PROJECT_OUT = LOCATE_OUT, PROJECT_INSIDE = LOCATE_IN, PROJECT_OUTSIDE = LOCATE_UNDECIDED;      // classes of the hit list
constexpr int PROJECT_SOLVED = 0, PROJECT_BEYOND = 1, PROJECT_FAILED = -1;
constexpr double PROJECT_SPAN = 0x1p-80;           // |z|^2 at or below it: row j lies in the span of the working set
constexpr double PROJECT_VIOLATED = 0x1p-44;       // of m_i: a row violated by less is satisfied (after the first step)
constexpr int PROJECT_LANES = LOCATE_WAVE;         // pairs per workgroup of the solve

// row i normalised: ah[N], returns b^_i
template <int N> GCS_INFORMED_EXACT_FN GCS_LOCATE_HD double project_row(const LocateRegions &R, int i, double *ah)
{
    GCS_INFORMED_EXACT_BODY
    const double *a = R.A + (size_t)i * N;
    double sq = 0.0;
#pragma unroll
    for (int k = 0; k < N; ++k) sq += a[k] * a[k];
    const double nrm = sqrt(sq);
#pragma unroll
    for (int k = 0; k < N; ++k) ah[k] = a[k] / nrm;
    return R.b[i] / nrm;
}
// g_i at x, and m_i
template <int N> GCS_LOCATE_HD double project_gap(const double *ah, double bh, const double *x, double *mag)
{
    double g = -bh, m = fabs(bh);
#pragma unroll
    for (int k = 0; k < N; ++k) {
        g = fma(ah[k], x[k], g);
        m = fma(fabs(ah[k]), fabs(x[k]), m);
    }
    *mag = m;
    return g;
}
GCS_LOCATE_HD bool project_finite(double v) { return fabs(v) < INFINITY; }

// the class of one pair: PROJECT_OUT (not a candidate), PROJECT_INSIDE or PROJECT_OUTSIDE
template <int N> GCS_INFORMED_EXACT_FN GCS_LOCATE_HD int project_classify(const LocateRegions &R, int region, const double *p, double radius)
{
    GCS_INFORMED_EXACT_BODY
    const int first = R.ptr[region], last = R.ptr[region + 1];
    const double reach = radius * (1.0 + 1e-9);
    bool inside = true;
    for (int i = first; i < last; ++i) {
        double ah[N], mag;
        const double bh = project_row<N>(R, i, ah);
        const double g = project_gap<N>(ah, bh, p, &mag);
        if (g > fma(0x1p-40, mag, reach)) return PROJECT_OUT;
        inside = inside && !(g > 0.0);
    }
    return inside ? PROJECT_INSIDE : PROJECT_OUTSIDE;
}
// ... of a lane's region (OUT past the end)
template <int N> GCS_LOCATE_HD int project_lane(const LocateRegions &R, int region, const double *p, double radius)
{
    return region >= 0 ? project_classify<N>(R, region, p, radius) : PROJECT_OUT;
}

// The working set of one solve.  Places k .. N-1: w = -1, u = 0, a zero row of Q, a unit row of L.
template <int N> struct ProjectSet {
    int k, w[N];
    double u[N], Q[N][N], L[N][N];
};
template <int N> GCS_LOCATE_HD void project_clear(ProjectSet<N> &S)
{
    S.k = 0;
#pragma unroll
    for (int i = 0; i < N; ++i) {
        S.w[i] = -1; S.u[i] = 0.0;
#pragma unroll
        for (int j = 0; j < N; ++j) { S.Q[i][j] = 0.0; S.L[i][j] = i == j ? 1.0 : 0.0; }
    }
}
// one more Gram-Schmidt row: c = Q v and v -= Q' c, one row of Q after the other; returns |v|^2 of what is left
template <int N> GCS_INFORMED_EXACT_FN GCS_LOCATE_HD double project_reduce(const ProjectSet<N> &S, double *v, double *c)
{
    GCS_INFORMED_EXACT_BODY
#pragma unroll
    for (int i = 0; i < N; ++i) {
        double dot = 0.0;
#pragma unroll
        for (int k = 0; k < N; ++k) dot += S.Q[i][k] * v[k];
        c[i] = dot;
#pragma unroll
        for (int k = 0; k < N; ++k) v[k] -= dot * S.Q[i][k];
    }
    double zz = 0.0;
#pragma unroll
    for (int k = 0; k < N; ++k) zz += v[k] * v[k];
    return zz;
}
// row `row` with multiplier u enters at place S.k (< N): v, c, zz as project_reduce left them
template <int N> GCS_INFORMED_EXACT_FN GCS_LOCATE_HD void project_enter(ProjectSet<N> &S, int row, double u, const double *v, const double *c, double zz)
{
    GCS_INFORMED_EXACT_BODY
    const double len = sqrt(zz);
    double q[N];
#pragma unroll
    for (int k = 0; k < N; ++k) q[k] = v[k] / len;
    // (selects, not a branch around the stores: a store under `i == S.k` in every place is one store at a run-time index to the
    // compiler, and the whole set would leave the registers for it)
#pragma unroll
    for (int i = 0; i < N; ++i) {
        const bool here = i == S.k;
        S.w[i] = here ? row : S.w[i];
        S.u[i] = here ? u : S.u[i];
#pragma unroll
        for (int k = 0; k < N; ++k) S.Q[i][k] = here ? q[k] : S.Q[i][k];
#pragma unroll
        for (int j = 0; j < N; ++j) S.L[i][j] = here ? (j < i ? c[j] : (j == i ? len : 0.0)) : S.L[i][j];
    }
    S.k += 1;
}
// the row at place `at` leaves: the later ones move up, L and Q are rebuilt from the rows that stay
template <int N> GCS_LOCATE_HD void project_leave(const LocateRegions &R, ProjectSet<N> &S, int at)
{
    int w[N];
    double u[N];
#pragma unroll
    for (int i = 0; i < N; ++i) {
        constexpr int last = N - 1;
        const int next = i < last ? i + 1 : last;      // (the place behind the working set is empty already)
        w[i] = i < at ? S.w[i] : (i < last ? S.w[next] : -1);
        u[i] = i < at ? S.u[i] : (i < last ? S.u[next] : 0.0);
    }
    const int k = S.k - 1;
    project_clear(S);
#pragma unroll
    for (int i = 0; i < N; ++i) {
        if (i >= k) continue;
        double v[N], c[N];
        (void)project_row<N>(R, w[i], v);
        const double zz = project_reduce<N>(S, v, c);
        project_enter<N>(S, w[i], u[i], v, c, zz);
    }
}
// r = L^-T c
template <int N> GCS_INFORMED_EXACT_FN GCS_LOCATE_HD void project_dual_direction(const ProjectSet<N> &S, const double *c, double *r)
{
    GCS_INFORMED_EXACT_BODY
#pragma unroll
    for (int i = N - 1; i >= 0; --i) {
        double t = c[i];
#pragma unroll
        for (int j = N - 1; j > i; --j) t -= S.L[j][i] * r[j];
        r[i] = t / S.L[i][i];
    }
}
// the end of a solve: the working rows hold at x up to the rounding of the steps, which is relative to |p|.  One correction by the
// minimum-norm solution of N dx = N x - b^ (dx = Q' L^-1 (N x - b^)) makes them hold up to the rounding of x itself
template <int N> GCS_INFORMED_EXACT_FN GCS_LOCATE_HD void project_polish(const LocateRegions &R, const ProjectSet<N> &S, double *x)
{
    GCS_INFORMED_EXACT_BODY
    double s[N], y[N];
#pragma unroll
    for (int i = 0; i < N; ++i) {
        double g = 0.0;
        if (i < S.k) {
            double ah[N], mag;
            const double bh = project_row<N>(R, S.w[i], ah);
            g = project_gap<N>(ah, bh, x, &mag);
        }
        s[i] = g;
    }
#pragma unroll
    for (int i = 0; i < N; ++i) {
        double t = s[i];
#pragma unroll
        for (int j = 0; j < i; ++j) t -= S.L[i][j] * y[j];
        y[i] = t / S.L[i][i];
    }
#pragma unroll
    for (int k = 0; k < N; ++k) {
        double acc = 0.0;
#pragma unroll
        for (int i = 0; i < N; ++i) acc += S.Q[i][k] * y[i];
        x[k] -= acc;
    }
}

// The projection of p onto `region`: x[N], *d and *iterations; returns the status.
template <int N> GCS_INFORMED_EXACT_FN GCS_LOCATE_HD int project_solve(const LocateRegions &R, int region, const double *p, double radius, int max_iter, double *x,
                                                                     double *d, int *iterations)
{
    GCS_INFORMED_EXACT_BODY
    const int first = R.ptr[region], last = R.ptr[region + 1];
    ProjectSet<N> S;
    project_clear(S);
#pragma unroll
    for (int k = 0; k < N; ++k) x[k] = p[k];
    int it = 0;
    bool failed = false;
    while (!failed) {
        // 1. the most violated row outside the working set
        int j = -1;
        double worst = 0.0;
        const double allow = it == 0 ? 0.0 : PROJECT_VIOLATED;
        for (int i = first; i < last; ++i) {
            bool working = false;
#pragma unroll
            for (int m = 0; m < N; ++m) working = working || S.w[m] == i;
            if (working) continue;
            double ah[N], mag;
            const double bh = project_row<N>(R, i, ah);
            const double g = project_gap<N>(ah, bh, x, &mag);
            if (!project_finite(g)) failed = true;
            if (g > allow * mag && g > worst) { worst = g; j = i; }
        }
        if (j < 0 || failed) break;
        double ah[N], uj = 0.0;
        const double bh = project_row<N>(R, j, ah);
        for (;;) {
            if (it >= max_iter) { failed = true; break; }
            ++it;
            // 2. the directions
            double z[N], c[N], r[N];
#pragma unroll
            for (int k = 0; k < N; ++k) z[k] = ah[k];
            const double zz = project_reduce<N>(S, z, c);
            project_dual_direction<N>(S, c, r);
            // 3. the steps
            double t2 = INFINITY;
            int leave = -1;
#pragma unroll
            for (int i = 0; i < N; ++i) {
                if (i < S.k && r[i] > 0.0) {
                    const double t = S.u[i] / r[i];
                    if (t < t2) { t2 = t; leave = i; }
                }
            }
            const bool spanned = S.k >= N || !(zz > PROJECT_SPAN);
            double t = t2;
            bool full = false;
            if (!spanned) {
                double mag;
                const double g = project_gap<N>(ah, bh, x, &mag);
                const double t1 = g > 0.0 ? g / zz : 0.0;
                full = !(t2 < t1);
                t = full ? t1 : t2;
#pragma unroll
                for (int k = 0; k < N; ++k) x[k] -= t * z[k];
            }
            if (!project_finite(t)) { failed = true; break; }      // (spanned and no r_i > 0: no step; or a NaN)
#pragma unroll
            for (int i = 0; i < N; ++i) S.u[i] -= t * r[i];
            uj += t;
            // 4. the working set
            if (full) { project_enter<N>(S, j, uj, z, c, zz); break; }
            project_leave<N>(R, S, leave);
        }
    }
    if (!failed && S.k > 0) project_polish<N>(R, S, x);
    *d = informed_distance(x, p, N);
    *iterations = it;
    bool finite = project_finite(*d);
#pragma unroll
    for (int k = 0; k < N; ++k) finite = finite && project_finite(x[k]);
    if (failed || !finite) return PROJECT_FAILED;
    return *d <= radius ? PROJECT_SOLVED : PROJECT_BEYOND;
}

// the point of list entry t: the q with hit_ptr[q] <= t < hit_ptr[q + 1]
GCS_LOCATE_HD long long project_point_of(const long long *hit_ptr, long long num_points, long long t)
{
    long long lo = 0, hi = num_points;      // hit_ptr[lo] <= t < hit_ptr[hi]
    while (hi - lo > 1) {
        const long long mid = lo + ((hi - lo) >> 1);
        if (hit_ptr[mid] <= t) lo = mid;
        else hi = mid;
    }
    return lo;
}

// one lane of the solve: list entry t
struct ProjectOut {
    double *distance, *nearest;      // [T], [T][N]
    int *status, *iterations;        // [T]
};
template <int N> GCS_LOCATE_HD void project_entry(const LocateRegions &R, const double *points, const double *radius, const long long *hit_ptr,
                                                  long long num_points, const int *hit_region, int max_iter, long long t, const ProjectOut &out)
{
    const long long q = project_point_of(hit_ptr, num_points, t);
    double p[N], x[N], d;
#pragma unroll
    for (int k = 0; k < N; ++k) p[k] = points[(size_t)q * N + k];
    int it;
    const int st = project_solve<N>(R, hit_region[t], p, radius[q], max_iter, x, &d, &it);
#pragma unroll
    for (int k = 0; k < N; ++k) out.nearest[(size_t)t * N + k] = x[k];
    out.distance[t] = d; out.status[t] = st; out.iterations[t] = it;
}

} // namespace gcsadmm_lp
