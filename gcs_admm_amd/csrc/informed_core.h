// informed_core.h -- the informed region set of a query: the rule shared by region_weight_kernel, region_path_kernel and
// informed_keep_kernel (scene_kernels.h) and their host build (tests/hostemu/informed_emu.cpp; the product path is the kernels).
//
// Contract, candidate path: a shortest path of query (s, g) on the region graph (query_graph_core.h: row_ptr, head; the graph is
// symmetric, so row v lists v's in-neighbours).  rs, rt: the ascending region lists under s and g.
//   weight    w[p] = |c_u - c_v|_2 of region edge p = (u, v) on the resident centres, the squares summed in ascending coordinate order,
//             every product and sum rounded on its own (no fused multiply-add);
//   init      init[r] = |s - c_r| for r in rs, +inf otherwise;
//   d         the fixed point of d[v] = min(init[v], min over p in row v of d[head[p]] + w[p]).  One pull-relaxation (informed_relax)
//             writes d[v] alone; values only fall from init, and a + w is monotone in a, so the fixed point is the same for every order
//             of the relaxations: rounds of them until one changes nothing;
//   goal      the r in rt that minimises d[r] + |c_r - g|, the smallest r among equals; that minimum is the cost of the polyline
//             s, c_r0, .., c_rk-1, g;
//   backtrack from the goal region: stop at a v with d[v] == init[v]; otherwise step to the smallest head u of row v with
//             d[u] + w[p] == d[v].  The path is reported from the start side to the goal side.
//   status    0 found; 1 no region of rs reaches one of rt (length 0, cost inf); 2 longer than max_len (length and cost are reported, no
//             region is); -1 the backtrack took more than P steps or found no step (a zero-weight cycle between regions with identical
//             centres).
//
// Contract, keep: lb(r) = dist(s, box_r) + dist(g, box_r) on the resident boxes, every side moved out by pad:
//   dist(p, box) = sqrt(sum_k max(lo_k - pad - p_k, 0, p_k - hi_k - pad)^2)   (a side opened to -inf / +inf contributes 0)
// and r is kept iff lb(r) <= bound (1 + 1e-9).  A region on an optimal path holds a point p of it, so lb(r) <= |s - p| + |p - g| <= L* <=
// bound for every bound that is the length of a feasible path; the rounding of the two distances and of the bound's own sum stays
// below (k + n + 4) 2^-52 relative, orders of magnitude under the 1e-9, which widens the set and never narrows it.  bound = +inf keeps all.
#pragma once
#include <cmath>
#include <string>
#include "query_graph_core.h"

namespace gcsadmm_lp {

// The sums of squares below are not contracted: the backtrack compares d[v] with a start distance it computes again, bit for bit, and
// the product must give the same bits at every site the compiler inlines a distance, on the device and on the host.
// (hipcc: a pragma at the head of the body; g++, the host build: an attribute of the function)
#if defined(__clang__)
#define GCS_INFORMED_EXACT_FN
#define GCS_INFORMED_EXACT_BODY _Pragma("clang fp contract(off)")
#else
#define GCS_INFORMED_EXACT_FN __attribute__((optimize("fp-contract=off")))
#define GCS_INFORMED_EXACT_BODY
#endif

constexpr int PATH_THREADS = 256;                  // lanes of region_path_kernel: lane t owns the vertices t, t + 256, ...
constexpr double INFORMED_SLACK = 1e-9;            // relative widening of the bound in the keep test
constexpr int PATH_FOUND = 0, PATH_NONE = 1, PATH_TOO_LONG = 2, PATH_CYCLE = -1;

// |a - b|_2 in dimension n, the squares summed in ascending coordinate order
GCS_INFORMED_EXACT_FN GCS_SWEEP_HD double informed_distance(const double *a, const double *b, int n)
{
    GCS_INFORMED_EXACT_BODY
    double sq = 0.0;
    for (int k = 0; k < n; ++k) {
        const double t = a[k] - b[k];
        sq += t * t;
    }
    return sqrt(sq);
}

// ---- candidate path ----
struct PathGraph {
    int P, n;
    const long long *row_ptr;       // [P + 1]
    const int *head;                // [E_R]
    const double *w;                // [E_R]
    const double *centers;          // [P][n]
};
struct PathQuery {
    const double *s, *g;            // [n]
    const int *rs, *rt;             // ascending
    int a, b;
};
// weight of region edge p (tail and head: the graph's arrays)
GCS_SWEEP_HD double informed_weight(const double *centers, int n, const int *tail, const int *head, long long p)
{
    return informed_distance(centers + (size_t)tail[p] * n, centers + (size_t)head[p] * n, n);
}
GCS_SWEEP_HD double informed_init(const PathGraph &g, const PathQuery &q, int v)
{
    const long long at = graph_lower_bound(q.rs, 0, q.a, v);
    return at < q.a && q.rs[at] == v ? informed_distance(q.s, g.centers + (size_t)v * g.n, g.n) : INFINITY;
}
// one pull-relaxation of vertex v: true iff d[v] fell.  The loads of a row do not depend on one another.
GCS_SWEEP_HD bool informed_relax(const PathGraph &g, double *d, int v)
{
    const double cur = d[v];
    double best = cur;
    const long long last = g.row_ptr[v + 1];
    for (long long p = g.row_ptr[v]; p < last; ++p) best = fmin(best, d[g.head[p]] + g.w[p]);
    if (!(best < cur)) return false;
    d[v] = best;
    return true;
}
// the goal region (-1: none is reached) and the cost of the centre polyline
GCS_SWEEP_HD int informed_goal(const PathGraph &g, const PathQuery &q, const double *d, double *cost)
{
    int goal = -1;
    double best = INFINITY;
    for (int j = 0; j < q.b; ++j) {
        const int r = q.rt[j];
        const double c = d[r] + informed_distance(g.centers + (size_t)r * g.n, q.g, g.n);
        if (c < best) { best = c; goal = r; }      // (ascending list, strict test: the smallest r among equals)
    }
    *cost = best;
    return goal;
}
// the vertex before v on the path (-1: v is where it starts; -2: no row entry explains d[v])
GCS_SWEEP_HD int informed_step(const PathGraph &g, const PathQuery &q, const double *d, int v)
{
    if (d[v] == informed_init(g, q, v)) return -1;
    const long long last = g.row_ptr[v + 1];
    for (long long p = g.row_ptr[v]; p < last; ++p)      // (heads ascending: the first match is the smallest)
        if (d[g.head[p]] + g.w[p] == d[v]) return g.head[p];
    return -2;
}
// the path into path_region[max_len] (start side first), its length and the status; one lane runs it once d has settled
GCS_SWEEP_HD int informed_backtrack(const PathGraph &g, const PathQuery &q, const double *d, int max_len, int *path_region, int *path_len, double *path_cost)
{
    *path_len = 0;
    const int goal = informed_goal(g, q, d, path_cost);
    if (goal < 0) return PATH_NONE;
    int len = 1;
    for (int v = goal;; ++len) {
        v = informed_step(g, q, d, v);
        if (v == -1) break;
        if (v < 0 || len >= g.P) return PATH_CYCLE;
    }
    *path_len = len;
    if (len > max_len) return PATH_TOO_LONG;
    for (int v = goal, at = len - 1; at >= 0; --at) {
        path_region[at] = v;
        if (at > 0) v = informed_step(g, q, d, v);
    }
    return PATH_FOUND;
}

// ---- keep ----
GCS_INFORMED_EXACT_FN GCS_SWEEP_HD double informed_box_distance(const double *p, const double *lo, const double *hi, int n, double pad)
{
    GCS_INFORMED_EXACT_BODY
    double sq = 0.0;
    for (int k = 0; k < n; ++k) {
        const double t = fmax(fmax(lo[k] - pad - p[k], 0.0), p[k] - hi[k] - pad);
        sq += t * t;
    }
    return sqrt(sq);
}
GCS_SWEEP_HD double informed_lower_bound(const double *s, const double *g, const double *lo, const double *hi, int n, double pad)
{
    return informed_box_distance(s, lo, hi, n, pad) + informed_box_distance(g, lo, hi, n, pad);
}
GCS_SWEEP_HD bool informed_keep(double lb, double bound) { return lb <= bound * (1.0 + INFORMED_SLACK); }

// ---- host side ----
constexpr long long PATH_WORKSPACE_BYTES = 256LL << 20;      // what d of one chunk of queries stays within
// queries per launch of region_path_kernel: as many rows of d as the workspace bound holds (one at least)
inline int informed_chunk(int P) { return (int)std::min<long long>(std::max(PATH_WORKSPACE_BYTES / (8LL * std::max(P, 1)), 1LL), QUERY_CHUNK_MAX); }
// what region_paths indexes with, checked before any launch
inline int informed_check_paths(int P, int n, int B, const double *points, const long long *term_ptr, const int *term_region, int max_len, std::string &err)
{
    if (B < 0) { err = "negative number of queries"; return QUERY_BAD_ARG; }
    if (max_len < 1) { err = "max_len must be at least 1"; return QUERY_BAD_ARG; }
    if (B == 0) return QUERY_OK;
    if (!points || !term_ptr) { err = "null points or term_ptr"; return QUERY_BAD_ARG; }
    for (size_t i = 0; i < 2 * (size_t)B * n; ++i)
        if (!std::isfinite(points[i])) { err = "point with a NaN or an inf coordinate"; return QUERY_BAD_ARG; }
    return query_check_terms(P, B, term_ptr, term_region, err);
}
inline int informed_check_keep(int n, int B, const double *points, const double *bound, double pad, std::string &err)
{
    if (B < 0) { err = "negative number of queries"; return QUERY_BAD_ARG; }
    if (!(pad == pad)) { err = "pad is NaN"; return QUERY_BAD_ARG; }
    if (B == 0) return QUERY_OK;
    if (!points || !bound) { err = "null points or bound"; return QUERY_BAD_ARG; }
    for (size_t i = 0; i < 2 * (size_t)B * n; ++i)
        if (!std::isfinite(points[i])) { err = "point with a NaN or an inf coordinate"; return QUERY_BAD_ARG; }
    for (int i = 0; i < B; ++i)
        if (!(bound[i] >= 0.0)) { err = "bound of query " + std::to_string(i) + " is NaN or negative"; return QUERY_BAD_ARG; }
    return QUERY_OK;
}

} // namespace gcsadmm_lp
