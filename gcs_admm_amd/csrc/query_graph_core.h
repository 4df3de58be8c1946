// query_graph_core.h -- the query graphs of a batch, assembled where the pair list lives: the pieces shared by the region-graph and
// query-graph kernels (polytope_lp.hip) and their host build (tests/hostemu/query_graph_emu.cpp; the product path is the kernels).
//
// Contract, region graph: from the resident pair list (pa < pb, any order, one flag each) the directed edges, both directions of every
// pair with a non-zero flag, sorted by (tail, head) -- scene.edge_arrays(pa, pb, flags) element for element -- with row_ptr[P + 1]
// (64-bit; row u holds the edges with tail u) and rev[E_R], the id of the opposite edge.  Four passes, no sort, no degree limit:
//   count    one thread per pair: the degree of both regions (integer adds: the sums do not depend on the order);
//   scan     exclusive, on the host (P integers; the total is known before anything is allocated);
//   scatter  one thread per pair: a slot of each row, in the order the threads arrive -- the tails are final (a row has one tail), the
//            heads are not;
//   place    one thread per edge: the head goes to "number of smaller heads in its row" in a second buffer, which is the same on every
//            run whatever order the scatter took;
//   reverse  one thread per edge (u, w): u is found in row w by bisection.
//
// Contract, query graph: what SceneQueries.graphs + graph._finish_graph build for one query, all seven arrays element for element.
// Vertices: 0 = 's', 1 = 't', r + 2 = region r.  rs, rt: the ascending region lists under start and goal, a = |rs|, b = |rt|; c = 1 iff
// the two point boxes meet.  lt(L, r) / le(L, r): entries of L below / not above r; in = le - lt.  T = 2c + a + b terminal edges leave s
// and t, so with the edges sorted by (tail, head):
//   s->t 0 (if c)     s->rs[i] c + i     t->s c + a (if c)     t->rt[j] 2c + a + j
//   r->s   row_ptr[r] + T + lt(rs, r) + lt(rt, r)        r->t   that + in(rs, r)
//   region edge p = (u, w)   p + T + le(rs, u) + le(rt, u)
//   inc_ptr: 0, 2(c + a), + 2(c + b), then inc_ptr[r + 2] = inc_ptr[2] + 2 row_ptr[r] + 2 lt(rs, r) + 2 lt(rt, r) for r = 0 .. P
// A vertex lists its incoming edges in edge order, then its outgoing ones: s [t->s], the r->s, [s->t], the s->r; t alike; region u with
// degree d: [s->u], [t->u], the d incoming region edges (the k-th is rev[row_ptr[u] + k]), [u->s], [u->t], the d outgoing ones.
// Work items of one query: one per region edge (it writes its own entry of the four edge arrays and the k-th incoming and the k-th
// outgoing slot of its TAIL, so lanes over consecutive edges write consecutive addresses in every array), one per entry of inc_ptr,
// one per terminal hit and one for the s-t pair.  Every entry is written exactly once, by plain stores.
#pragma once
#include <string>
#include "box_sweep_core.h"

namespace gcsadmm_lp {

// ---- region graph ----
struct RegionBuild {
    int P;
    long long T;                    // pairs
    const int *pa, *pb;
    const unsigned char *flag;      // [T]
    int *count;                     // [P] degrees (count pass); slots taken so far (scatter pass, zeroed in between)
    const long long *row_ptr;       // [P + 1]
    int *unsorted;                  // [E_R] heads as the scatter left them
    int *tail, *head, *rev;         // [E_R]
};
// the value before the add; the threads of the host build run one after the other
GCS_SWEEP_HD int graph_take(int *counter)
{
#if defined(__HIP_DEVICE_COMPILE__)
    return atomicAdd(counter, 1);
#else
    return (*counter)++;
#endif
}
// thread t of T
GCS_SWEEP_HD void region_count(const RegionBuild &g, long long t)
{
    if (!g.flag[t]) return;
    graph_take(g.count + g.pa[t]);
    graph_take(g.count + g.pb[t]);
}
GCS_SWEEP_HD void region_scatter(const RegionBuild &g, long long t)
{
    if (!g.flag[t]) return;
    const int a = g.pa[t], b = g.pb[t];
    const long long ea = g.row_ptr[a] + graph_take(g.count + a), eb = g.row_ptr[b] + graph_take(g.count + b);
    g.tail[ea] = a; g.unsorted[ea] = b;
    g.tail[eb] = b; g.unsorted[eb] = a;
}
// thread p of E_R (a pair listed twice would tie: the earlier slot goes first, and both hold the same value)
GCS_SWEEP_HD void region_place(const RegionBuild &g, long long p)
{
    const int u = g.tail[p], w = g.unsorted[p];
    const long long first = g.row_ptr[u], last = g.row_ptr[u + 1];
    long long below = 0;
    for (long long j = first; j < last; ++j) below += (g.unsorted[j] < w || (g.unsorted[j] == w && j < p)) ? 1 : 0;
    g.head[first + below] = w;
}
// first index of the ascending v[first .. last) whose value is not below key
GCS_SWEEP_HD long long graph_lower_bound(const int *v, long long first, long long last, int key)
{
    while (first < last) {
        const long long mid = first + ((last - first) >> 1);
        if (v[mid] < key) first = mid + 1;
        else last = mid;
    }
    return first;
}
GCS_SWEEP_HD void region_reverse(const RegionBuild &g, long long p)
{
    const int u = g.tail[p], w = g.head[p];
    g.rev[p] = (int)graph_lower_bound(g.head, g.row_ptr[w], g.row_ptr[w + 1], u);
}

// ---- query graph ----
struct RegionGraph {
    int P;
    long long E;                    // E_R
    const long long *row_ptr;
    const int *tail, *head, *rev;
};
struct QueryTerms {
    const int *rs, *rt;             // ascending
    int a, b, c;
};
struct QueryArrays {                // of one query, or of the first query of a chunk
    int *edge_tail, *edge_head, *inc_ptr, *inc_edge, *inc_out, *edge_inc_tail, *edge_inc_head;
};
// a region against the two hit lists
struct TermRanks {
    int lt, le;                     // lt(rs, r) + lt(rt, r); le(rs, r) + le(rt, r)
    int in_s, in_t;
};
GCS_SWEEP_HD TermRanks query_ranks(const QueryTerms &k, int r)
{
    const int lt_s = (int)graph_lower_bound(k.rs, 0, k.a, r), lt_t = (int)graph_lower_bound(k.rt, 0, k.b, r);
    TermRanks x;
    x.in_s = lt_s < k.a && k.rs[lt_s] == r ? 1 : 0;
    x.in_t = lt_t < k.b && k.rt[lt_t] == r ? 1 : 0;
    x.lt = lt_s + lt_t;
    x.le = x.lt + x.in_s + x.in_t;
    return x;
}
GCS_SWEEP_HD long long query_terminal_edges(const QueryTerms &k) { return 2LL * k.c + k.a + k.b; }
GCS_SWEEP_HD long long query_edges(long long region_edges, int a, int b, int c) { return region_edges + 2LL * (a + b) + 2LL * c; }
GCS_SWEEP_HD long long query_inc1(const QueryTerms &k) { return 2LL * (k.c + k.a); }
GCS_SWEEP_HD long long query_inc2(const QueryTerms &k) { return query_inc1(k) + 2LL * (k.c + k.b); }
// first incidence of region r
GCS_SWEEP_HD long long query_region_base(const RegionGraph &g, const QueryTerms &k, int r, const TermRanks &x)
{
    return query_inc2(k) + 2 * g.row_ptr[r] + 2LL * x.lt;
}
// id of r -> s (whether it is there or not: the first edge of tail r + 2)
GCS_SWEEP_HD long long query_down_id(const RegionGraph &g, const QueryTerms &k, int r, const TermRanks &x)
{
    return g.row_ptr[r] + query_terminal_edges(k) + x.lt;
}
GCS_SWEEP_HD void query_put_edge(const QueryArrays &o, long long e, long long tail, long long head, long long at_tail, long long at_head)
{
    o.edge_tail[e] = (int)tail; o.edge_head[e] = (int)head;
    o.edge_inc_tail[e] = (int)at_tail; o.edge_inc_head[e] = (int)at_head;
    o.inc_edge[at_tail] = (int)e; o.inc_out[at_tail] = 1;
    o.inc_edge[at_head] = (int)e; o.inc_out[at_head] = 0;
}

// region edge p = (u, w): its entry of the edge arrays, and the k-th incoming and outgoing slot of u (k = p - row_ptr[u])
GCS_SWEEP_HD void query_region_edge(const RegionGraph &g, const QueryTerms &t, const QueryArrays &o, long long p)
{
    const int u = g.tail[p], w = g.head[p];
    const long long q = g.rev[p];                       // the edge (w, u)
    const TermRanks xu = query_ranks(t, u), xw = query_ranks(t, w);
    const long long T = query_terminal_edges(t);
    const long long k = p - g.row_ptr[u], d = g.row_ptr[u + 1] - g.row_ptr[u], h = xu.in_s + xu.in_t;
    const long long base = query_region_base(g, t, u, xu);
    const long long in_slot = base + h + k, out_slot = base + 2 * h + d + k;
    const long long e = p + T + xu.le, back = q + T + xw.le;
    o.edge_tail[e] = u + 2; o.edge_head[e] = w + 2;
    o.edge_inc_tail[e] = (int)out_slot;
    o.edge_inc_head[e] = (int)(query_region_base(g, t, w, xw) + xw.in_s + xw.in_t + (q - g.row_ptr[w]));
    o.inc_edge[in_slot] = (int)back; o.inc_out[in_slot] = 0;
    o.inc_edge[out_slot] = (int)e; o.inc_out[out_slot] = 1;
}
// entry v of inc_ptr, v = 0 .. P + 2
GCS_SWEEP_HD void query_inc_ptr(const RegionGraph &g, const QueryTerms &t, const QueryArrays &o, int v)
{
    long long at = v == 0 ? 0 : query_inc1(t);
    if (v >= 2) {
        const int r = v - 2;
        at = query_region_base(g, t, r, query_ranks(t, r));      // (r = P: the rank of a region above all, the end of the last row)
    }
    o.inc_ptr[v] = (int)at;
}
// terminal item j: j < a the two edges between s and rs[j]; j < a + b those between t and rt[j - a]; j = a + b the s-t pair (if c)
GCS_SWEEP_HD void query_terminal(const RegionGraph &g, const QueryTerms &t, const QueryArrays &o, int j)
{
    const long long inc1 = query_inc1(t);
    if (j == t.a + t.b) {
        if (!t.c) return;
        query_put_edge(o, 0, 0, 1, t.c + t.a, inc1);                             // s -> t
        query_put_edge(o, t.c + t.a, 1, 0, inc1 + t.c + t.b, 0);                 // t -> s
        return;
    }
    const bool from_s = j < t.a;
    const int i = from_s ? j : j - t.a, r = from_s ? t.rs[i] : t.rt[i];
    const TermRanks x = query_ranks(t, r);
    const long long d = g.row_ptr[r + 1] - g.row_ptr[r], h = x.in_s + x.in_t;
    const long long base = query_region_base(g, t, r, x), down = query_down_id(g, t, r, x);
    if (from_s) {
        query_put_edge(o, t.c + i, 0, r + 2, 2LL * t.c + t.a + i, base);                          // s -> r
        query_put_edge(o, down, r + 2, 0, base + h + d, t.c + i);                                 // r -> s
    } else {
        query_put_edge(o, 2LL * t.c + t.a + i, 1, r + 2, inc1 + 2LL * t.c + t.b + i, base + x.in_s);      // t -> r
        query_put_edge(o, down + x.in_s, r + 2, 1, base + h + d + x.in_s, inc1 + t.c + i);               // r -> t
    }
}
GCS_SWEEP_HD long long query_items(const RegionGraph &g, int a, int b) { return g.E + g.P + 3 + a + b + 1; }
// work item x of query_items(): the region edges first (the bulk of the stores), inc_ptr, the terminals
GCS_SWEEP_HD void query_item(const RegionGraph &g, const QueryTerms &t, const QueryArrays &o, long long x)
{
    if (x < g.E) query_region_edge(g, t, o, x);
    else if (x < g.E + g.P + 3) query_inc_ptr(g, t, o, (int)(x - g.E));
    else if (x < query_items(g, t.a, t.b)) query_terminal(g, t, o, (int)(x - g.E - g.P - 3));
}

// the queries of a call as the kernel reads them: points 0 .. B-1 the starts, B .. 2B-1 the goals
struct QueryBatch {
    int B;
    const long long *term_ptr;      // [2B + 1]
    const int *term_region;
    const unsigned char *st;        // [B]
    const long long *edge_off;      // [B + 1]
};
GCS_SWEEP_HD QueryTerms query_terms(const QueryBatch &q, int i)
{
    QueryTerms t;
    t.rs = q.term_region + q.term_ptr[i]; t.a = (int)(q.term_ptr[i + 1] - q.term_ptr[i]);
    t.rt = q.term_region + q.term_ptr[q.B + i]; t.b = (int)(q.term_ptr[q.B + i + 1] - q.term_ptr[q.B + i]);
    t.c = q.st[i] ? 1 : 0;
    return t;
}
// the arrays of query i in buffers that begin with query `first`
GCS_SWEEP_HD QueryArrays query_arrays(const QueryArrays &chunk, const QueryBatch &q, int P, int first, int i)
{
    const size_t e = (size_t)(q.edge_off[i] - q.edge_off[first]);
    return QueryArrays{chunk.edge_tail + e, chunk.edge_head + e, chunk.inc_ptr + (size_t)(i - first) * ((size_t)P + 3), chunk.inc_edge + 2 * e,
                       chunk.inc_out + 2 * e, chunk.edge_inc_tail + e, chunk.edge_inc_head + e};
}

// ---- host side ----
constexpr int QUERY_OK = 0, QUERY_BAD_ARG = 1, QUERY_UNSUPPORTED = 2;      // GCSADMM_OK, GCSADMM_ERR_BAD_ARG, GCSADMM_ERR_UNSUPPORTED
constexpr long long QUERY_WORKSPACE_BYTES = 256LL << 20;                   // what the library's own choice of chunk_queries stays within
constexpr int QUERY_CHUNK_MAX = 65535;                                     // grid.y

// exclusive scan of the degrees; false: some query graph on these regions could have 2 E above 2^31 - 1 (E <= E_R + 4 P + 2)
inline bool region_scan(const int *count, int P, long long *row_ptr)
{
    long long s = 0;
    for (int r = 0; r < P; ++r) {
        row_ptr[r] = s;
        s += count[r];
    }
    row_ptr[P] = s;
    return 2 * (s + 4LL * P + 2) <= (long long)INT32_MAX;
}
// bytes of the seven arrays of one query with E edges
inline long long query_bytes(long long E, int P) { return 4 * (8 * E + P + 3); }
// queries per launch: the caller's number, or as many of the largest possible query as the workspace bound holds (one at least)
inline int query_chunk(int P, long long region_edges, int asked)
{
    const long long fit = QUERY_WORKSPACE_BYTES / query_bytes(region_edges + 4LL * P + 2, P);
    const long long chunk = asked > 0 ? asked : std::max(fit, 1LL);
    return (int)std::min<long long>(chunk, QUERY_CHUNK_MAX);
}
// The hit lists of B > 0 queries (term_ptr not null): 2 B segments from 0 on, each strictly ascending within [0, P).
inline int query_check_terms(int P, int B, const long long *term_ptr, const int *term_region, std::string &err)
{
    if (B > INT32_MAX / 2) { err = "more than 2^30 queries"; return QUERY_UNSUPPORTED; }
    const long long points = 2LL * B;
    if (term_ptr[0] != 0) { err = "term_ptr[0] != 0"; return QUERY_BAD_ARG; }
    for (long long p = 0; p < points; ++p)
        if (term_ptr[p + 1] < term_ptr[p]) { err = "term_ptr is not non-decreasing"; return QUERY_BAD_ARG; }
    if (term_ptr[points] > (long long)INT32_MAX) { err = "more than 2^31 - 1 hits"; return QUERY_UNSUPPORTED; }
    if (term_ptr[points] > 0 && !term_region) { err = "null term_region"; return QUERY_BAD_ARG; }
    for (long long p = 0; p < points; ++p)
        for (long long j = term_ptr[p]; j < term_ptr[p + 1]; ++j) {
            const int r = term_region[j];
            if (r < 0 || r >= P) { err = "hit list of point " + std::to_string(p) + ": region index out of range"; return QUERY_BAD_ARG; }
            if (j > term_ptr[p] && term_region[j - 1] >= r) {
                err = "hit list of point " + std::to_string(p) + " is not strictly ascending"; return QUERY_BAD_ARG;
            }
        }
    return QUERY_OK;
}
// Everything the kernel will index with, checked before any launch.  *max_items: the most work items of one query.
inline int query_check(int P, long long region_edges, const QueryBatch &q, int chunk_queries, std::string &err, long long *max_items)
{
    *max_items = 0;
    if (q.B < 0 || chunk_queries < 0) { err = "negative number of queries or chunk_queries"; return QUERY_BAD_ARG; }
    if (q.B == 0) return QUERY_OK;
    if (!q.term_ptr || !q.st || !q.edge_off) { err = "null term_ptr, st_adjacent or edge_off"; return QUERY_BAD_ARG; }
    if (const int rc = query_check_terms(P, q.B, q.term_ptr, q.term_region, err)) return rc;
    if (q.edge_off[0] < 0) { err = "edge_off starts below 0"; return QUERY_BAD_ARG; }
    for (int i = 0; i < q.B; ++i) {
        if (q.st[i] > 1) { err = "st_adjacent of query " + std::to_string(i) + " is neither 0 nor 1"; return QUERY_BAD_ARG; }
        const QueryTerms t = query_terms(q, i);
        if (q.edge_off[i + 1] - q.edge_off[i] != query_edges(region_edges, t.a, t.b, t.c)) {
            err = "edge_off of query " + std::to_string(i) + " is not its number of edges"; return QUERY_BAD_ARG;
        }
        *max_items = std::max(*max_items, region_edges + P + 3 + t.a + t.b + 1);
    }
    return QUERY_OK;
}

} // namespace gcsadmm_lp
