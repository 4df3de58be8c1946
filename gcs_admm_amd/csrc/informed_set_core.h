// informed_set_core.h -- the informed region set of a query whose start and goal are SETS: the rule shared by terminal_set_path_kernel and
// terminal_set_keep_kernel (scene_kernels.h) and their host build (tests/hostemu/informed_set_emu.cpp; the product path is the kernels).
// informed_core.h has the rule for points; this header changes what is measured from, and ends the search early.
//
// A terminal is a box [tlo, thi]; a point is the box with tlo == thi.  S, G: the start and the goal box; rs, rt: the ascending lists of
// the regions that meet them.
//   dist(c, T)   = sqrt(sum_k max(tlo_k - c_k, 0, c_k - thi_k)^2), the distance of a point to a box, summed in ascending k;
//   gap(T, box)  = sqrt(sum_k max(lo_k - pad - thi_k, 0, tlo_k - hi_k - pad)^2), the distance between two boxes, the region's sides moved
//                  out by pad (a side opened to -inf / +inf contributes 0).
// No product or sum of either is contracted.  With tlo == thi == p the first maximum is |p - c|, whose square is that of p - c, and the
// second is the expression of informed_box_distance: on degenerate boxes every result below has the bits of informed_core.h.
//
// Contract, candidate path: that of informed_core.h (weights, relaxation, tie rules, the four statuses) with
//   init      init[r] = dist(c_r, S) for r in rs, +inf otherwise;
//   goal      the r in rt that minimises d[r] + dist(c_r, G), the smallest r among equals;
//   backtrack the start test d[v] == init[v] computes init[v] a second time.
// The cost is the length of the polyline s*, c_r0, .., c_rk-1, g* with s* the point of S nearest c_r0 and g* that of G nearest c_rk-1.
//
// Bounded search.  U: the smallest goal cost d[r] + dist(c_r, G), r in rt, seen so far (+inf at first).  A relaxation stores its minimum
// only when that is below d[v] AND not above U (set_relax); the rounds end, as in informed_core.h, with one that stored nothing.  U may
// lag behind d: any value that was the goal cost of a d already written only admits more than the newest one.
//   Status, path, length and cost are those of the unbounded rule; d[v] is the unbounded fixed point wherever that is <= cost, and at
//   least that value (or +inf) elsewhere; without a reachable goal U stays +inf and the search is the unbounded one.
// Why: every U is the cost of a real polyline, so U >= C*, the optimum.  A vertex whose true distance is <= C* has, on the chain that
// realises it, predecessors of no larger distance (w >= 0, a float add is monotone); by induction none of their updates is rejected,
// and a round that stores nothing has them final.  A vertex whose stored value is not final has a true value above C*: it neither wins
// nor ties the goal choice, and explains no d[v] <= C* in the backtrack.  A local query on a large graph settles in the few rounds its
// own path needs, where the unbounded rule runs until the whole component has settled.
//
// Contract, keep: r is kept iff gap(S, box_r) + gap(G, box_r) <= bound (1 + 1e-9).  A region on an optimal path holds a point p of
// it, and the path runs from some s* in S to some g* in G: gap(S, box_r) + gap(G, box_r) <= |s* - p| + |p - g*| <= L* <= bound for
// every bound that is the length of a feasible path.  The slack covers the rounding, as in informed_core.h.
#pragma once
#include "informed_core.h"

namespace gcsadmm_lp {

struct SetQuery {
    const double *slo, *shi, *glo, *ghi;      // [n] each
    const int *rs, *rt;                       // ascending
    int a, b;
};

// query i of a batch: lo, hi [2 B][n], the start boxes and then the goal boxes; the hit lists as query_graph_core.h has them (none: the keep rule)
GCS_SWEEP_HD SetQuery set_query(const double *lo, const double *hi, const long long *term_ptr, const int *term_region, int B, int n, int i)
{
    SetQuery q;
    q.slo = lo + (size_t)i * n; q.shi = hi + (size_t)i * n; q.glo = lo + (size_t)(B + i) * n; q.ghi = hi + (size_t)(B + i) * n;
    q.rs = q.rt = nullptr; q.a = q.b = 0;
    if (term_ptr) {
        q.rs = term_region + term_ptr[i]; q.a = (int)(term_ptr[i + 1] - term_ptr[i]);
        q.rt = term_region + term_ptr[B + i]; q.b = (int)(term_ptr[B + i + 1] - term_ptr[B + i]);
    }
    return q;
}

// ---- distances ----
GCS_INFORMED_EXACT_FN GCS_SWEEP_HD double set_point_distance(const double *c, const double *tlo, const double *thi, int n)
{
    GCS_INFORMED_EXACT_BODY
    double sq = 0.0;
    for (int k = 0; k < n; ++k) {
        const double t = fmax(fmax(tlo[k] - c[k], 0.0), c[k] - thi[k]);
        sq += t * t;
    }
    return sqrt(sq);
}
GCS_INFORMED_EXACT_FN GCS_SWEEP_HD double set_box_gap(const double *tlo, const double *thi, const double *lo, const double *hi, int n, double pad)
{
    GCS_INFORMED_EXACT_BODY
    double sq = 0.0;
    for (int k = 0; k < n; ++k) {
        const double t = fmax(fmax(lo[k] - pad - thi[k], 0.0), tlo[k] - hi[k] - pad);
        sq += t * t;
    }
    return sqrt(sq);
}

// ---- candidate path ----
GCS_SWEEP_HD double set_init(const PathGraph &g, const SetQuery &q, int v)
{
    const long long at = graph_lower_bound(q.rs, 0, q.a, v);
    return at < q.a && q.rs[at] == v ? set_point_distance(g.centers + (size_t)v * g.n, q.slo, q.shi, g.n) : INFINITY;
}
// the cost of the polyline that ends in region r of rt
GCS_SWEEP_HD double set_goal_cost(const PathGraph &g, const SetQuery &q, const double *d, int r)
{
    return d[r] + set_point_distance(g.centers + (size_t)r * g.n, q.glo, q.ghi, g.n);
}
// does the goal cost c lower the bound?  (the one test of every fold into it, on the device and on the host)
GCS_SWEEP_HD bool set_lowers(double c, double bound_now) { return c < bound_now; }
// one pull-relaxation of vertex v under the bound U (informed_relax has the loop): true iff d[v] fell
GCS_SWEEP_HD bool set_relax(const PathGraph &g, double *d, int v, double U)
{
    const double cur = d[v];
    double best = cur;
    const long long last = g.row_ptr[v + 1];
    for (long long p = g.row_ptr[v]; p < last; ++p) best = fmin(best, d[g.head[p]] + g.w[p]);
    if (!(best < cur && best <= U)) return false;
    d[v] = best;
    return true;
}
GCS_SWEEP_HD int set_goal(const PathGraph &g, const SetQuery &q, const double *d, double *cost)
{
    int goal = -1;
    double best = INFINITY;
    for (int j = 0; j < q.b; ++j) {
        const double c = set_goal_cost(g, q, d, q.rt[j]);
        if (c < best) { best = c; goal = q.rt[j]; }      // (ascending list, strict test: the smallest r among equals)
    }
    *cost = best;
    return goal;
}
// informed_step, the start test on the set's init
GCS_SWEEP_HD int set_step(const PathGraph &g, const SetQuery &q, const double *d, int v)
{
    if (d[v] == set_init(g, q, v)) return -1;
    const long long last = g.row_ptr[v + 1];
    for (long long p = g.row_ptr[v]; p < last; ++p)
        if (d[g.head[p]] + g.w[p] == d[v]) return g.head[p];
    return -2;
}
// informed_backtrack on set_goal and set_step
GCS_SWEEP_HD int set_backtrack(const PathGraph &g, const SetQuery &q, const double *d, int max_len, int *path_region, int *path_len, double *path_cost)
{
    *path_len = 0;
    const int goal = set_goal(g, q, d, path_cost);
    if (goal < 0) return PATH_NONE;
    int len = 1;
    for (int v = goal;; ++len) {
        v = set_step(g, q, d, v);
        if (v == -1) break;
        if (v < 0 || len >= g.P) return PATH_CYCLE;
    }
    *path_len = len;
    if (len > max_len) return PATH_TOO_LONG;
    for (int v = goal, at = len - 1; at >= 0; --at) {
        path_region[at] = v;
        if (at > 0) v = set_step(g, q, d, v);
    }
    return PATH_FOUND;
}

// ---- keep ----
GCS_SWEEP_HD double set_lower_bound(const SetQuery &q, const double *lo, const double *hi, int n, double pad)
{
    return set_box_gap(q.slo, q.shi, lo, hi, n, pad) + set_box_gap(q.glo, q.ghi, lo, hi, n, pad);
}

// ---- host side ----
// terminal boxes lo, hi [2 B][n]: finite, lo <= hi
inline int set_check_boxes(int n, int B, const double *lo, const double *hi, std::string &err)
{
    for (size_t i = 0; i < 2 * (size_t)B * n; ++i) {
        if (!std::isfinite(lo[i]) || !std::isfinite(hi[i])) { err = "box with a NaN or an inf coordinate"; return QUERY_BAD_ARG; }
        if (lo[i] > hi[i]) { err = "box " + std::to_string(i / (size_t)n) + " has lo above hi"; return QUERY_BAD_ARG; }
    }
    return QUERY_OK;
}
// what region_paths_sets indexes with, checked before any launch
inline int set_check_paths(int P, int n, int B, const double *lo, const double *hi, const long long *term_ptr, const int *term_region, int max_len,
                           std::string &err)
{
    if (B < 0) { err = "negative number of queries"; return QUERY_BAD_ARG; }
    if (max_len < 1) { err = "max_len must be at least 1"; return QUERY_BAD_ARG; }
    if (B == 0) return QUERY_OK;
    if (!lo || !hi || !term_ptr) { err = "null lo, hi or term_ptr"; return QUERY_BAD_ARG; }
    if (const int rc = set_check_boxes(n, B, lo, hi, err)) return rc;
    return query_check_terms(P, B, term_ptr, term_region, err);
}
inline int set_check_keep(int n, int B, const double *lo, const double *hi, const double *bound, double pad, std::string &err)
{
    if (B < 0) { err = "negative number of queries"; return QUERY_BAD_ARG; }
    if (!(pad == pad)) { err = "pad is NaN"; return QUERY_BAD_ARG; }
    if (B == 0) return QUERY_OK;
    if (!lo || !hi || !bound) { err = "null lo, hi or bound"; return QUERY_BAD_ARG; }
    if (const int rc = set_check_boxes(n, B, lo, hi, err)) return rc;
    for (int i = 0; i < B; ++i)
        if (!(bound[i] >= 0.0) || !std::isfinite(bound[i])) { err = "bound of query " + std::to_string(i) + " is not finite or negative"; return QUERY_BAD_ARG; }
    return QUERY_OK;
}

} // namespace gcsadmm_lp
