// Host build of the region-graph and query-graph kernels of csrc/polytope_lp.hip (query_graph_core.h): the steps of
// gcsadmm_scene_build_region_graph, gcsadmm_scene_read_region_graph and gcsadmm_scene_query_graphs on a pair list handed in, with the
// threads of a launch run one after the other, the same checks, the same chunks and the same copies out of the chunk buffers.
// Test infrastructure: never shipped, never timed.
#include <algorithm>
#include <cstring>
#include <string>
#include <vector>
#include "query_graph_core.h"
using namespace gcsadmm_lp;

namespace {

struct Emu {
    int P = 0;
    std::vector<int> pa, pb;
    std::vector<unsigned char> flag;              // the resident flags
    std::vector<long long> row_ptr;
    std::vector<int> tail, head, rev;
    bool have_graph = false;
    std::string err;
    RegionGraph graph() const { return RegionGraph{P, row_ptr.empty() ? 0 : row_ptr.back(), row_ptr.data(), tail.data(), head.data(), rev.data()}; }
};

} // namespace

extern "C" {

void *qg_emu_create(int P, long long T, const int *pa, const int *pb, const unsigned char *flag)
{
    Emu *e = new Emu;
    e->P = P;
    e->pa.assign(pa, pa + T); e->pb.assign(pb, pb + T); e->flag.assign(flag, flag + T);
    return e;
}
void qg_emu_destroy(void *h) { delete (Emu *)h; }
const char *qg_emu_last_error(void *h) { return ((Emu *)h)->err.c_str(); }
// what an edit or a new narrow phase does to the graph
void qg_emu_invalidate(void *h) { ((Emu *)h)->have_graph = false; }

int qg_emu_build(void *h, const unsigned char *overlap, long long *num_edges)
{
    Emu *e = (Emu *)h;
    const int P = e->P;
    const long long T = (long long)e->pa.size();
    e->have_graph = false;
    RegionBuild g{};
    g.P = P; g.T = T; g.pa = e->pa.data(); g.pb = e->pb.data(); g.flag = overlap ? overlap : e->flag.data();
    std::vector<int> count((size_t)P + 1, 0);
    std::vector<long long> row_ptr((size_t)P + 1);
    g.count = count.data();
    for (long long t = 0; t < T; ++t) region_count(g, t);
    if (!region_scan(count.data(), P, row_ptr.data())) { e->err = "too many region edges for 32-bit incidence indices"; return QUERY_UNSUPPORTED; }
    const size_t E = (size_t)row_ptr[(size_t)P];
    std::vector<int> unsorted(E + 1), tail(E + 1, -1), head(E + 1, -1), rev(E + 1, -1);
    std::fill(count.begin(), count.end(), 0);
    g.row_ptr = row_ptr.data(); g.unsorted = unsorted.data(); g.tail = tail.data(); g.head = head.data(); g.rev = rev.data();
    for (long long t = 0; t < T; ++t) region_scatter(g, t);
    for (size_t p = E; p-- > 0;) region_place(g, (long long)p);      // (any order of the threads gives the same arrays)
    for (size_t p = 0; p < E; ++p) region_reverse(g, (long long)p);
    tail.resize(E); head.resize(E); rev.resize(E);
    e->row_ptr.swap(row_ptr); e->tail.swap(tail); e->head.swap(head); e->rev.swap(rev);
    e->have_graph = true;
    if (num_edges) *num_edges = (long long)E;
    return QUERY_OK;
}

int qg_emu_read(void *h, long long *row_ptr, int *edge_tail, int *edge_head, int *reverse)
{
    Emu *e = (Emu *)h;
    if (!e->have_graph) { e->err = "no resident region graph"; return QUERY_BAD_ARG; }
    if (row_ptr) std::copy(e->row_ptr.begin(), e->row_ptr.end(), row_ptr);
    if (edge_tail) std::copy(e->tail.begin(), e->tail.end(), edge_tail);
    if (edge_head) std::copy(e->head.begin(), e->head.end(), edge_head);
    if (reverse) std::copy(e->rev.begin(), e->rev.end(), reverse);
    return QUERY_OK;
}

int qg_emu_query(void *h, int num_queries, const long long *term_ptr, const int *term_region, const unsigned char *st_adjacent, int chunk_queries,
                 const long long *edge_off, int *edge_tail, int *edge_head, int *inc_ptr, int *inc_edge, int *inc_out, int *edge_inc_tail,
                 int *edge_inc_head)
{
    Emu *e = (Emu *)h;
    if (!e->have_graph) { e->err = "no resident region graph"; return QUERY_BAD_ARG; }
    const RegionGraph g = e->graph();
    const QueryBatch q{num_queries, term_ptr, term_region, st_adjacent, edge_off};
    long long max_items = 0;
    if (const int rc = query_check(g.P, g.E, q, chunk_queries, e->err, &max_items)) return rc;
    const int chunk = query_chunk(g.P, g.E, chunk_queries);
    const size_t V1 = (size_t)g.P + 3;
    for (int first = 0; first < num_queries; first += chunk) {
        const int count = std::min(chunk, num_queries - first);
        const size_t E = (size_t)(edge_off[first + count] - edge_off[first]);
        // the chunk's buffers, filled with a value no entry takes: an entry that is not written shows.  (SLACK entries behind each: the
        // seeded errors of test_query_graph.py move an edge id or a slot up by two at the most, and must not leave the buffer)
        constexpr size_t SLACK = 8;
        std::vector<int> et(E + SLACK, -7), eh(E + SLACK, -7), ip(count * V1, -7), ie(2 * E + SLACK, -7), io(2 * E + SLACK, -7), eit(E + SLACK, -7),
            eih(E + SLACK, -7);
        const QueryArrays buf{et.data(), eh.data(), ip.data(), ie.data(), io.data(), eit.data(), eih.data()};
        for (int y = 0; y < count; ++y) {                          // blockIdx.y
            const int i = first + y;
            const QueryTerms t = query_terms(q, i);
            const QueryArrays o = query_arrays(buf, q, g.P, first, i);
            for (long long x = 0; x < max_items; ++x) query_item(g, t, o, x);
        }
        const size_t at = (size_t)edge_off[first];
        std::memcpy(edge_tail + at, et.data(), 4 * E); std::memcpy(edge_head + at, eh.data(), 4 * E);
        std::memcpy(edge_inc_tail + at, eit.data(), 4 * E); std::memcpy(edge_inc_head + at, eih.data(), 4 * E);
        std::memcpy(inc_edge + 2 * at, ie.data(), 8 * E); std::memcpy(inc_out + 2 * at, io.data(), 8 * E);
        std::memcpy(inc_ptr + (size_t)first * V1, ip.data(), 4 * count * V1);
    }
    return QUERY_OK;
}

// region_scan as the library calls it: 1 if every query graph on a region graph with these degrees keeps 32-bit indices
int qg_emu_scan(const int *count, int P, long long *row_ptr) { return region_scan(count, P, row_ptr) ? 1 : 0; }
int qg_emu_chunk(int P, long long region_edges, int asked) { return query_chunk(P, region_edges, asked); }

} // extern "C"
