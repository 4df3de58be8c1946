// halo_plan_emu.cpp -- what a vertex partition decides on the host (gcs_admm_amd/csrc/halo_plan.h), for tests/test_halo_plan.py: the
// plan is made from a descriptor as gcsadmm_create makes it (create_plan.h), then the halo checks, the message layout and the overlap
// split are run on it and read back by name.  Linked with wg_sizes.cpp built at 256 and at 512 threads, as plan_emu.cpp is.
// Test-only; the product has no path into it.
#include <cstring>

#include "halo_plan.h"
#include "terminal_region.h"

long long gcsadmm_terminal_ws_doubles(int n, int facets, int live_edges) { return gcs_term::terminal_ws_doubles(n, facets, live_edges); }
long long gcsadmm_terminal_record_doubles(int n, int facets, int live_edges) { return gcs_term::terminal_record_doubles(n, facets, live_edges); }

using namespace gcsadmm_k;

static CreatePlan g_plan;
static int g_V = 0, g_NI = 0;
static HaloPlan g_halo;
static OverlapSplit g_split;
static std::string g_err;

static int copy_out(const std::vector<int> &v, size_t count, int *out, int capacity)
{
    for (size_t i = 0; i < count && (int)i < capacity; ++i) out[i] = v[i];
    return (int)count;
}

// the plan of a handle as gcsadmm_create would make it (a device is taken to be present); its status, the message: halo_emu_error
extern "C" int halo_emu_plan(const gcsadmm_graph_desc *g)
{
    g_err.clear();
    gcsadmm_status st = check_graph_desc(g, g_err);
    if (st == GCSADMM_OK) st = make_create_plan(*g, g_plan, g_err);
    if (st == GCSADMM_OK) { g_V = g->num_vertices; g_NI = g->num_incidences; }
    return (int)st;
}

extern "C" const char *halo_emu_error() { return g_err.c_str(); }

// gcsadmm_check_halo on a handle with that plan and nothing attached
extern "C" int halo_emu_check(int rank, int world, const gcsadmm_halo_desc *hd)
{
    g_err.clear();
    return (int)check_halo(g_plan.col_owned, g_NI, rank, world, hd, g_err);
}

// the layout of the packed message for c words per column; returns n_send, the arrays by name through halo_emu_vec
extern "C" int halo_emu_layout(int c, const gcsadmm_halo_desc *hd)
{
    g_halo = make_halo_plan(c, hd);
    return g_halo.n_send;
}

// "n_recv", or an array of the last layout ("peers", "peer_cnt", "peer_off": one per peer; "send_cols", "base", "stride": one per sent
// column) or of the last split ("ids"): copies at most `capacity` entries and returns the count; -1: no such name
extern "C" int halo_emu_vec(const char *name, int *out, int capacity)
{
    const HaloPlan &H = g_halo;
    if (!std::strcmp(name, "n_recv")) return H.n_recv;
    if (!std::strcmp(name, "peers")) return copy_out(H.peers, H.peers.size(), out, capacity);
    if (!std::strcmp(name, "peer_cnt")) return copy_out(H.peer_cnt, H.peer_cnt.size(), out, capacity);
    if (!std::strcmp(name, "peer_off")) return copy_out(H.peer_off, H.peer_off.size(), out, capacity);
    if (!std::strcmp(name, "send_cols")) return copy_out(H.send_cols, H.send_cols.size(), out, capacity);
    if (!std::strcmp(name, "base")) return copy_out(H.base, (size_t)H.n_send, out, capacity);
    if (!std::strcmp(name, "stride")) return copy_out(H.stride, (size_t)H.n_send, out, capacity);
    if (!std::strcmp(name, "ids")) return copy_out(g_split.ids, g_split.ids.size(), out, capacity);
    return -1;
}

// the overlap split of that plan for a send list and a gcsadmm_set_overlap mode; n_wg / n_split < 0: the plan's own counts of
// workgroup-program and split-form vertices.  Returns n_wave_b, the ids through halo_emu_vec("ids")
extern "C" int halo_emu_split(const int *send_cols, int n_send, int mode, int n_wg, int n_split)
{
    const std::vector<int> cols(send_cols, send_cols + n_send);
    g_split = overlap_split(g_plan, g_V, cols, mode, n_wg < 0 ? (int)g_plan.wg_vtx.size() : n_wg, n_split < 0 ? (int)g_plan.split_vtx.size() : n_split);
    return g_split.n_wave_b;
}
