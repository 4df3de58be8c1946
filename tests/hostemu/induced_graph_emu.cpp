// Host build of the induced-graph kernels of csrc/scene_kernels.h (induced_graph_core.h): the steps of gcsadmm_scene_induced_sizes and
// gcsadmm_scene_induced_query_graphs on a region graph handed in, with the lanes of a workgroup run one after the other -- forwards
// or backwards --, the same checks, the same chunks, the same table of slabs and the same copies out of the chunk buffers.
// Test infrastructure: never shipped, never timed.
#include <algorithm>
#include <cstring>
#include <string>
#include <vector>
#include "induced_graph_core.h"
using namespace gcsadmm_lp;

namespace {

struct Emu {
    int P = 0;
    bool backwards = false, fresh = true;
    std::vector<long long> row_ptr;
    std::vector<int> tail, head, rev;
    std::string err;
    RegionGraph graph() const { return RegionGraph{P, row_ptr.back(), row_ptr.data(), tail.data(), head.data(), rev.data()}; }
    template <class F> void lanes(F &&f) const
    {
        for (int k = 0; k < INDUCED_TILE; ++k) f(backwards ? INDUCED_TILE - 1 - k : k);
    }
};

constexpr int FILL = -7;            // no entry takes it: one that is not written shows
constexpr size_t SLACK = 8;

// the buffers of one chunk
struct Chunk {
    std::vector<int> newidx, kept, deg, full_ptr, rank, tail, head, rev;
    std::vector<long long> row_ptr;
    std::vector<InducedQuery> table;
    const unsigned char *keep = nullptr;
    InducedWorkspace workspace()
    {
        return InducedWorkspace{keep, newidx.data(), kept.data(), deg.data(), row_ptr.data(), full_ptr.data(), rank.data(), tail.data(), head.data(), rev.data()};
    }
};

// induced_count_kernel, workgroup y
void count_query(const Emu &e, const InducedQuery &q, int *z)
{
    const RegionGraph g = e.graph();
    TileCarry below;
    std::vector<InducedCount> sum(INDUCED_TILE, InducedCount{0, 0});
    int flag[INDUCED_TILE], within[INDUCED_TILE], edges[INDUCED_TILE], ranks[INDUCED_TILE];
    for (int base = 0; base < g.P; base += INDUCED_TILE) {
        e.lanes([&](int t) { flag[t] = induced_flag(q, g.P, base + t); });
        const int total = induced_tile_scan(flag, within);
        e.lanes([&](int t) { if (base + t < g.P) induced_number(g, q, base + t, flag[t], below.at(within[t]), sum[(size_t)t]); });
        below.next(total);
    }
    e.lanes([&](int t) { edges[t] = sum[(size_t)t].edges; ranks[t] = sum[(size_t)t].ranks; });
    z[0] = below.sum; z[1] = induced_tile_scan(edges, within); z[2] = induced_tile_scan(ranks, within);
}

// induced_build_kernel, workgroup of query i
void build_query(const Emu &e, const InducedQuery &q, const QueryBatch &b, int i, int *term_new)
{
    const RegionGraph g = e.graph();
    const int kept = q.kept_count;
    TileCarry first, ranks;
    int deg[INDUCED_TILE], full[INDUCED_TILE], e_within[INDUCED_TILE], f_within[INDUCED_TILE];
    for (int base = 0; base < kept; base += INDUCED_TILE) {
        e.lanes([&](int t) {
            deg[t] = base + t < kept ? q.deg[base + t] : 0;
            full[t] = base + t < kept ? induced_full_degree(g, q, base + t) : 0;
        });
        const int edges = induced_tile_scan(deg, e_within), all = induced_tile_scan(full, f_within);
        e.lanes([&](int t) { if (base + t < kept) induced_row(g, q, base + t, first.at(e_within[t]), ranks.at(f_within[t])); });
        first.next(edges); ranks.next(all);
    }
    q.row_ptr[kept] = first.sum;
    const int hits = induced_hits(b, i);
    e.lanes([&](int t) { for (int k = t; k < hits; k += INDUCED_TILE) induced_term(b, i, q.newidx, term_new, k); });
    e.lanes([&](int t) { for (int j = t; j < kept; j += INDUCED_TILE) induced_reverse(g, q, j); });      // (behind the barrier)
}

int count_chunk(Emu &e, const InducedBatch &q, int first, int count, Chunk &c, int *sizes)
{
    const size_t cells = (size_t)count * e.P + 1;
    c.newidx.assign(cells, FILL); c.kept.assign(cells, FILL); c.deg.assign(cells, FILL);
    c.keep = q.keep + (size_t)first * e.P;
    c.table.resize((size_t)count);
    induced_table(c.workspace(), e.P, count, nullptr, c.table.data());
    for (int y = 0; y < count; ++y) count_query(e, c.table[(size_t)y], sizes + (size_t)INDUCED_SIZES * y);
    return QUERY_OK;
}

int counts(Emu &e, const InducedBatch &q, int chunk_queries, int &chunk, Chunk &c, std::vector<int> &sizes)
{
    if (!e.fresh) { e.err = "no resident region graph, or one from before an edit"; return QUERY_BAD_ARG; }
    if (const int rc = induced_check(e.P, q, chunk_queries, e.err)) return rc;
    if (q.B == 0) return QUERY_OK;
    sizes.resize((size_t)INDUCED_SIZES * q.B);
    chunk = induced_chunk(e.P, e.row_ptr.back(), chunk_queries);
    for (int first = 0; first < q.B; first += chunk) count_chunk(e, q, first, std::min(chunk, q.B - first), c, sizes.data() + (size_t)INDUCED_SIZES * first);
    return QUERY_OK;
}

} // namespace

extern "C" {

void *ige_create(int P, const long long *row_ptr, const int *tail, const int *head, const int *rev, int backwards)
{
    Emu *e = new Emu;
    const size_t E = (size_t)row_ptr[P];
    e->P = P; e->backwards = backwards != 0;
    e->row_ptr.assign(row_ptr, row_ptr + P + 1);
    e->tail.assign(tail, tail + E); e->head.assign(head, head + E); e->rev.assign(rev, rev + E);
    return e;
}
void ige_destroy(void *h) { delete (Emu *)h; }
const char *ige_last_error(void *h) { return ((Emu *)h)->err.c_str(); }
// what an edit does to the graph
void ige_invalidate(void *h) { ((Emu *)h)->fresh = false; }
int ige_chunk(int P, long long region_edges, int asked) { return induced_chunk(P, region_edges, asked); }

int ige_sizes(void *h, int num_queries, const unsigned char *keep, const long long *term_ptr, const int *term_region, const unsigned char *st_adjacent,
              int *num_kept, long long *num_edges)
{
    Emu *e = (Emu *)h;
    const InducedBatch q{num_queries, keep, term_ptr, term_region, st_adjacent};
    if (num_queries > 0 && (!num_kept || !num_edges)) { e->err = "null output array"; return QUERY_BAD_ARG; }
    std::vector<int> sizes;
    Chunk c;
    int chunk = 0;
    if (const int rc = counts(*e, q, 0, chunk, c, sizes)) return rc;
    const QueryBatch b{q.B, q.term_ptr, q.term_region, q.st, nullptr};
    for (int i = 0; i < num_queries; ++i) {
        const QueryTerms t = query_terms(b, i);
        num_kept[i] = sizes[(size_t)INDUCED_SIZES * i];
        num_edges[i] = query_edges(sizes[(size_t)INDUCED_SIZES * i + 1], t.a, t.b, t.c);
    }
    return QUERY_OK;
}

int ige_graphs(void *h, int num_queries, const unsigned char *keep, const long long *term_ptr, const int *term_region, const unsigned char *st_adjacent,
               int chunk_queries, const long long *vertex_off, const long long *edge_off, int *edge_tail, int *edge_head, int *inc_ptr, int *inc_edge,
               int *inc_out, int *edge_inc_tail, int *edge_inc_head)
{
    Emu *e = (Emu *)h;
    const InducedBatch q{num_queries, keep, term_ptr, term_region, st_adjacent};
    const int B = num_queries;
    if (B > 0 && (!vertex_off || !edge_off || !edge_tail || !edge_head || !inc_ptr || !inc_edge || !inc_out || !edge_inc_tail || !edge_inc_head)) {
        e->err = "null vertex_off, edge_off or output array"; return QUERY_BAD_ARG;
    }
    std::vector<int> sizes, again;
    Chunk c;
    int chunk = 0;
    if (const int rc = counts(*e, q, chunk_queries, chunk, c, sizes)) return rc;
    if (B == 0) return QUERY_OK;
    if (const int rc = induced_check_offsets(q, sizes.data(), vertex_off, edge_off, e->err)) return rc;
    std::vector<int> term_new((size_t)term_ptr[2 * (size_t)B] + 1, FILL);
    const QueryBatch scene_terms{B, term_ptr, term_region, st_adjacent, edge_off}, new_terms{B, term_ptr, term_new.data(), st_adjacent, edge_off};
    again.resize((size_t)INDUCED_SIZES * std::min(chunk, B));
    for (int first = 0; first < B; first += chunk) {
        const int count = std::min(chunk, B - first);
        if (chunk < B) count_chunk(*e, q, first, count, c, again.data());
        const int *z = sizes.data() + (size_t)INDUCED_SIZES * first;
        const InducedTotals n = induced_totals(z, count);
        c.row_ptr.assign(n.kept + (size_t)count, FILL); c.full_ptr.assign(n.kept + 1, FILL); c.rank.assign(n.ranks + 1, FILL);
        c.tail.assign(n.edges + 1, FILL); c.head.assign(n.edges + 1, FILL); c.rev.assign(n.edges + 1, FILL);
        induced_table(c.workspace(), e->P, count, z, c.table.data());
        // what the build kernel indexes with: a seeded error in the renumbering must not leave the region graph
        for (int y = 0; y < count; ++y) {
            const InducedQuery &s = c.table[(size_t)y];
            for (int j = 0; j < s.kept_count; ++j)
                if (s.kept[j] < 0 || s.kept[j] >= e->P || (j > 0 && s.kept[j - 1] >= s.kept[j]) || s.newidx[s.kept[j]] != j) {
                    e->err = "host build: the kept regions are not listed ascending, each at its new index"; return 99;
                }
        }
        for (int y = 0; y < count; ++y) build_query(*e, c.table[(size_t)y], scene_terms, first + y, term_new.data());
        // what the query kernel indexes with, beyond the counts: a seeded error in the lists or the heads must not leave the buffers
        for (int y = 0; y < count; ++y) {
            const InducedQuery &s = c.table[(size_t)y];
            const QueryTerms t = query_terms(new_terms, first + y);
            for (int k = 0; k < t.a + t.b; ++k) {
                const int *list = k < t.a ? t.rs : t.rt;
                const int at = k < t.a ? k : k - t.a;
                if (list[at] < 0 || list[at] >= s.kept_count || (at > 0 && list[at - 1] >= list[at])) {
                    e->err = "host build: a renumbered hit list is not strictly ascending within the kept regions"; return 99;
                }
            }
            for (long long p = 0; p < s.edges; ++p)
                if (s.head[p] < 0 || s.head[p] >= s.kept_count || s.tail[p] < 0 || s.tail[p] >= s.kept_count) {
                    e->err = "host build: an induced edge leaves the kept regions"; return 99;
                }
        }
        const size_t at = (size_t)edge_off[first], E = (size_t)(edge_off[first + count] - edge_off[first]);
        const size_t v_at = (size_t)vertex_off[first], V = (size_t)(vertex_off[first + count] - vertex_off[first]);
        std::vector<int> et(E + SLACK, FILL), eh(E + SLACK, FILL), ip(V + SLACK, FILL), ie(2 * E + SLACK, FILL), io(2 * E + SLACK, FILL), eit(E + SLACK, FILL),
            eih(E + SLACK, FILL);
        const QueryArrays buf{et.data(), eh.data(), ip.data(), ie.data(), io.data(), eit.data(), eih.data()};
        long long max_items = 0;
        for (int y = 0; y < count; ++y)
            max_items = std::max(max_items, query_items(induced_region_graph(c.table[(size_t)y]), induced_hits(scene_terms, first + y), 0));
        for (int y = 0; y < count; ++y) {                          // blockIdx.y
            const int i = first + y;
            const RegionGraph g = induced_region_graph(c.table[(size_t)y]);
            const QueryTerms t = query_terms(new_terms, i);
            const QueryArrays o = induced_arrays(buf, new_terms, vertex_off, first, i);
            for (long long k = 0; k < max_items; ++k) {
                const long long x = e->backwards ? max_items - 1 - k : k;
                if (x < query_items(g, t.a, t.b)) query_item(g, t, o, x);
            }
        }
        std::memcpy(edge_tail + at, et.data(), 4 * E); std::memcpy(edge_head + at, eh.data(), 4 * E);
        std::memcpy(edge_inc_tail + at, eit.data(), 4 * E); std::memcpy(edge_inc_head + at, eih.data(), 4 * E);
        std::memcpy(inc_edge + 2 * at, ie.data(), 8 * E); std::memcpy(inc_out + 2 * at, io.data(), 8 * E);
        std::memcpy(inc_ptr + v_at, ip.data(), 4 * V);
    }
    return QUERY_OK;
}

} // extern "C"
