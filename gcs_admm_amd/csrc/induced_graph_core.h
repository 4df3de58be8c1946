// induced_graph_core.h -- the query graphs of a batch on each query's own kept regions, assembled where the region graph lives: the
// pieces shared by the induced-graph kernels (scene_kernels.h, polytope_lp.hip) and their host build
// (tests/hostemu/induced_graph_emu.cpp; the product path is the kernels).
//
// Contract, query i with flags keep[0 .. P) (any non-zero byte keeps a region): new[r] is the number of kept regions below r, P' the
// number kept, and the induced region graph is the one SceneQueries._host_graph(keep) masks and renumbers out of the whole edge list:
// the edges (u, w) with both ends kept, as (new[u], new[w]), in the order they had -- rows by new[u], heads ascending, because the
// renumbering is monotone --, with row_ptr'[P' + 1] and rev'.  The query graph on it is query_graph_core.h's, unchanged: query_item is
// handed a RegionGraph of the induced arrays and hit lists new[rs], new[rt] (ascending for the same reason).
//
// One 256-lane workgroup per query, three kernels, every entry written once by a plain store, no atomics (every count is one row's):
//   count    walks the P flags in tiles of 256: an exclusive scan of a tile (inside a wavefront by shuffles, the four wavefronts
//            through one LDS stage), carried into the next tile, gives new[r]; the lane of a kept region r lists it (kept[new[r]] = r)
//            and counts the kept heads of its own row (deg).  P', E' = sum of deg and D = sum of the kept rows' unpruned degrees go to
//            the host, which lays out the slabs and checks the caller's offsets before anything is written to them;
//   build    walks the P' kept rows in tiles: scans of deg and of the unpruned degrees place row j (row_ptr'[j]) and its ranks; the lane
//            of row j writes tail', head' and, for EVERY edge of the unpruned row, its rank among the row's kept heads.  After one
//            barrier the reverse edges: for edge p = (u, w), rev[p] lies in row w, which is kept whenever p is, so its rank was
//            written: rev'[p'] = row_ptr'[new[w]] + rank of rev[p].  The hit lists are renumbered here too;
//   query    query_item on the induced arrays: query_graph_kernel with one RegionGraph and one item count per query, from the table.
// Per query the device reads the P flags and the rows of the kept regions, and nothing else: no pass over all E_R edges.
#pragma once
#include <vector>
#include "query_graph_core.h"

namespace gcsadmm_lp {

constexpr int INDUCED_TILE = 256, INDUCED_WAVE = 64;      // lanes of a workgroup, of a wavefront

// one query and its slabs of the workspace: what the count kernel fills, then what the host lays out from its counts
struct InducedQuery {
    const unsigned char *keep;      // [P]
    int *newidx;                    // [P] new[r]
    int *kept, *deg;                // [P'] (room for P): the kept regions ascending, the kept heads of each one's row
    int kept_count;                 // P'
    long long edges;                // E'
    long long *row_ptr;             // [P' + 1]
    int *full_ptr;                  // [P'] where the ranks of row j begin: the unpruned degrees of the rows before it
    int *rank;                      // [D]
    int *tail, *head, *rev;         // [E']
};
struct InducedCount {               // what a lane adds up over its regions
    int edges, ranks;
};
// A running exclusive scan over tiles: the place inside the tile plus what the tiles before summed to.
struct TileCarry {
    int sum = 0;
    GCS_SWEEP_HD int at(int within) const { return sum + within; }
    GCS_SWEEP_HD void next(int tile_total) { sum += tile_total; }
};

// ---- the 256 lanes together: the exclusive scan of one tile.  Wave intrinsics and LDS on the device; the host build scans the lanes'
// values in a loop (a plain C++ compiler) ----
#if defined(__HIPCC__)
// lane threadIdx.x hands in v: the sum of the lanes below it, and in `total` that of all 256.  part: four ints of LDS.  Every lane of
// the workgroup calls it, the same number of times.
__device__ __forceinline__ int induced_tile_scan(int v, int *part, int &total)
{
    const int lane = (int)threadIdx.x % INDUCED_WAVE, wave = (int)threadIdx.x / INDUCED_WAVE;
    int x = v;                                                  // inclusive, inside the wavefront
    for (int off = 1; off < INDUCED_WAVE; off <<= 1) {
        const int below = __shfl_up(x, off, INDUCED_WAVE);
        if (lane >= off) x += below;
    }
    __syncthreads();                                            // (the scan before has read part[])
    if (lane == INDUCED_WAVE - 1) part[wave] = x;
    __syncthreads();
    int before = 0;
    total = 0;
    for (int k = 0; k < INDUCED_TILE / INDUCED_WAVE; ++k) {
        const int s = part[k];
        before += k < wave ? s : 0;
        total += s;
    }
    return before + x - v;
}
#else
inline int induced_tile_scan(const int *v, int *within)
{
    int s = 0;
    for (int t = 0; t < INDUCED_TILE; ++t) {
        within[t] = s;
        s += v[t];
    }
    return s;
}
#endif

// ---- count ----
GCS_SWEEP_HD int induced_flag(const InducedQuery &q, int P, int r) { return r < P && q.keep[r] ? 1 : 0; }
// kept heads of row u
GCS_SWEEP_HD int induced_degree(const RegionGraph &g, const InducedQuery &q, int u)
{
    int d = 0;
    for (long long p = g.row_ptr[u]; p < g.row_ptr[u + 1]; ++p) d += q.keep[g.head[p]] ? 1 : 0;
    return d;
}
// region r < P with `below` kept regions below it
GCS_SWEEP_HD void induced_number(const RegionGraph &g, const InducedQuery &q, int r, int flag, int below, InducedCount &sum)
{
    q.newidx[r] = below;
    if (!flag) return;
    const int d = induced_degree(g, q, r);
    q.kept[below] = r; q.deg[below] = d;
    sum.edges += d;
    sum.ranks += (int)(g.row_ptr[r + 1] - g.row_ptr[r]);
}

// ---- build ----
GCS_SWEEP_HD int induced_full_degree(const RegionGraph &g, const InducedQuery &q, int j)
{
    const int u = q.kept[j];
    return (int)(g.row_ptr[u + 1] - g.row_ptr[u]);
}
// kept row j, which begins at edge `first` of the induced graph and whose ranks begin at `ranks`
GCS_SWEEP_HD void induced_row(const RegionGraph &g, const InducedQuery &q, int j, int first, int ranks)
{
    const int u = q.kept[j];
    const long long row = g.row_ptr[u], end = g.row_ptr[u + 1];
    q.row_ptr[j] = first; q.full_ptr[j] = ranks;
    int k = 0;
    for (long long p = row; p < end; ++p) {
        const int w = g.head[p];
        q.rank[ranks + (p - row)] = k;
        if (!q.keep[w]) continue;
        q.tail[first + k] = j; q.head[first + k] = q.newidx[w];
        ++k;
    }
}
// the reverse edges of kept row j (after every row of the query is written)
GCS_SWEEP_HD void induced_reverse(const RegionGraph &g, const InducedQuery &q, int j)
{
    const int u = q.kept[j];
    const long long row = g.row_ptr[u], end = g.row_ptr[u + 1];
    for (long long p = row; p < end; ++p) {
        const int w = g.head[p];
        if (!q.keep[w]) continue;
        const int jw = q.newidx[w];
        const long long back = g.rev[p] - g.row_ptr[w];      // the place of (w, u) in the unpruned row w
        q.rev[q.row_ptr[j] + q.rank[q.full_ptr[j] + (p - row)]] = (int)(q.row_ptr[jw] + q.rank[q.full_ptr[jw] + back]);
    }
}
// hit k of query i's a + b: the start's list, then the goal's, into term_new at the place it has in term_region
GCS_SWEEP_HD void induced_term(const QueryBatch &b, int i, const int *newidx, int *term_new, int k)
{
    const int a = (int)(b.term_ptr[i + 1] - b.term_ptr[i]);
    if (k < a) {
        const long long s_at = b.term_ptr[i] + k;
        term_new[s_at] = newidx[b.term_region[s_at]];
    } else {
        const long long g_at = b.term_ptr[b.B + i] + (k - a);
        term_new[g_at] = newidx[b.term_region[g_at]];
    }
}
GCS_SWEEP_HD int induced_hits(const QueryBatch &b, int i)
{
    return (int)(b.term_ptr[i + 1] - b.term_ptr[i]) + (int)(b.term_ptr[b.B + i + 1] - b.term_ptr[b.B + i]);
}

// ---- query ----
GCS_SWEEP_HD RegionGraph induced_region_graph(const InducedQuery &q)
{
    return RegionGraph{q.kept_count, q.edges, q.row_ptr, q.tail, q.head, q.rev};
}
// the arrays of query i in buffers that begin with query `first`: its inc_ptr has P'_i + 3 entries, at vertex_off
GCS_SWEEP_HD QueryArrays induced_arrays(const QueryArrays &chunk, const QueryBatch &b, const long long *vertex_off, int first, int i)
{
    const size_t e = (size_t)(b.edge_off[i] - b.edge_off[first]), v = (size_t)(vertex_off[i] - vertex_off[first]);
    return QueryArrays{chunk.edge_tail + e, chunk.edge_head + e, chunk.inc_ptr + v, chunk.inc_edge + 2 * e, chunk.inc_out + 2 * e,
                       chunk.edge_inc_tail + e, chunk.edge_inc_head + e};
}

// ---- host side ----
struct InducedBatch {               // the caller's arrays
    int B;
    const unsigned char *keep;      // [B][P]
    const long long *term_ptr;      // [2 B + 1]
    const int *term_region;
    const unsigned char *st;        // [B]
};
constexpr int INDUCED_SIZES = 3;    // per query from the count kernel: P', E', D

// Everything that can be decided without the counts, before any launch.
inline int induced_check(int P, const InducedBatch &q, int chunk_queries, std::string &err)
{
    if (q.B < 0 || chunk_queries < 0) { err = "negative number of queries or chunk_queries"; return QUERY_BAD_ARG; }
    if (q.B == 0) return QUERY_OK;
    if (!q.keep || !q.term_ptr || !q.st) { err = "null keep, term_ptr or st_adjacent"; return QUERY_BAD_ARG; }
    if (const int rc = query_check_terms(P, q.B, q.term_ptr, q.term_region, err)) return rc;
    for (int i = 0; i < q.B; ++i) {
        if (q.st[i] > 1) { err = "st_adjacent of query " + std::to_string(i) + " is neither 0 nor 1"; return QUERY_BAD_ARG; }
        for (const int point : {i, q.B + i})
            for (long long j = q.term_ptr[point]; j < q.term_ptr[point + 1]; ++j)
                if (!q.keep[(size_t)i * P + q.term_region[j]]) {
                    err = "query " + std::to_string(i) + ": hit region " + std::to_string(q.term_region[j]) + " is not kept"; return QUERY_BAD_ARG;
                }
    }
    return QUERY_OK;
}
// The caller's offsets against the counts: before anything is written to the caller's arrays.
inline int induced_check_offsets(const InducedBatch &q, const int *sizes, const long long *vertex_off, const long long *edge_off, std::string &err)
{
    if (vertex_off[0] < 0 || edge_off[0] < 0) { err = "vertex_off or edge_off starts below 0"; return QUERY_BAD_ARG; }
    const QueryBatch b{q.B, q.term_ptr, q.term_region, q.st, edge_off};
    for (int i = 0; i < q.B; ++i) {
        const QueryTerms t = query_terms(b, i);
        const int *z = sizes + (size_t)INDUCED_SIZES * i;
        if (vertex_off[i + 1] - vertex_off[i] != z[0] + 3LL) {
            err = "vertex_off of query " + std::to_string(i) + " is not its number of kept regions + 3"; return QUERY_BAD_ARG;
        }
        if (edge_off[i + 1] - edge_off[i] != query_edges(z[1], t.a, t.b, t.c)) {
            err = "edge_off of query " + std::to_string(i) + " is not its number of edges"; return QUERY_BAD_ARG;
        }
    }
    return QUERY_OK;
}
// Queries per launch by query_chunk's rule, for the largest query there can be (every region kept): the flags, the three arrays of
// the count, the induced graph with its ranks, and the seven arrays of the result.
inline int induced_chunk(int P, long long region_edges, int asked)
{
    const long long one = 13LL * P + 8 * (P + 1LL) + 4LL * P + 16 * region_edges + query_bytes(region_edges + 4LL * P + 2, P);
    const long long chunk = asked > 0 ? asked : std::max(QUERY_WORKSPACE_BYTES / one, 1LL);
    return (int)std::min<long long>(chunk, QUERY_CHUNK_MAX);
}

// the workspace of one chunk; every slab of a query is a piece of one of these
struct InducedWorkspace {
    const unsigned char *keep;      // [count][P]
    int *newidx, *kept, *deg;       // [count][P]
    long long *row_ptr;             // [sum of P' + 1]
    int *full_ptr;                  // [sum of P']
    int *rank;                      // [sum of D]
    int *tail, *head, *rev;         // [sum of E']
};
struct InducedTotals {              // what a chunk's second part needs room for
    size_t kept = 0, edges = 0, ranks = 0;
};
inline InducedTotals induced_totals(const int *sizes, int count)
{
    InducedTotals n;
    for (int y = 0; y < count; ++y) {
        n.kept += (size_t)sizes[INDUCED_SIZES * y]; n.edges += (size_t)sizes[INDUCED_SIZES * y + 1]; n.ranks += (size_t)sizes[INDUCED_SIZES * y + 2];
    }
    return n;
}
// The table of a chunk.  sizes == nullptr: for the count kernel (the slabs of fixed size alone); else: every slab, laid out one query
// behind the other from the counts [count][INDUCED_SIZES].
inline void induced_table(const InducedWorkspace &w, int P, int count, const int *sizes, InducedQuery *table)
{
    InducedTotals at;
    for (int y = 0; y < count; ++y) {
        const size_t fixed = (size_t)y * P;
        InducedQuery q{};
        q.keep = w.keep + fixed; q.newidx = w.newidx + fixed; q.kept = w.kept + fixed; q.deg = w.deg + fixed;
        if (sizes) {
            q.kept_count = sizes[INDUCED_SIZES * y]; q.edges = sizes[INDUCED_SIZES * y + 1];
            q.row_ptr = w.row_ptr + at.kept + y; q.full_ptr = w.full_ptr + at.kept; q.rank = w.rank + at.ranks;
            q.tail = w.tail + at.edges; q.head = w.head + at.edges; q.rev = w.rev + at.edges;
            at.kept += (size_t)q.kept_count; at.edges += (size_t)q.edges; at.ranks += (size_t)sizes[INDUCED_SIZES * y + 2];
        }
        table[y] = q;
    }
}

} // namespace gcsadmm_lp
