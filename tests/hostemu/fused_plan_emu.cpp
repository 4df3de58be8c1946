// fused_plan_emu.cpp -- the fused-tail decision of gcsadmm_create (gcs_admm_amd/csrc/create_plan.h, CreatePlan::fused_tail) and the
// LDS request of the launch that carries the tail (step_args.h wg_launch_lds_bytes), on the host, for tests/test_fused_tail_plan.py.
// Linked with wg_sizes.cpp built at 256 and at 512 threads, as plan_emu.cpp is.  Test-only; the product has no path into it.
#include <cstring>

#include "create_plan.h"
#include "terminal_region.h"

long long gcsadmm_terminal_ws_doubles(int n, int facets, int live_edges) { return gcs_term::terminal_ws_doubles(n, facets, live_edges); }
long long gcsadmm_terminal_record_doubles(int n, int facets, int live_edges) { return gcs_term::terminal_record_doubles(n, facets, live_edges); }

static gcsadmm_k::CreatePlan g_plan;
static std::string g_err;

extern "C" int fused_plan_make(const gcsadmm_graph_desc *g)
{
    g_err.clear();
    gcsadmm_status st = gcsadmm_k::check_graph_desc(g, g_err);
    if (st == GCSADMM_OK) st = gcsadmm_k::make_create_plan(*g, g_plan, g_err);
    return (int)st;
}

extern "C" const char *fused_plan_error() { return g_err.c_str(); }

// field of the last plan, or what the launch derives from it; -1: no such field
extern "C" int fused_plan_get(const char *name)
{
    const gcsadmm_k::CreatePlan &p = g_plan;
    const struct { const char *name; int value; } fields[] = {
        {"fused_tail", p.fused_tail}, {"edge_blocks", p.edge_blocks}, {"n_waves", p.n_waves()}, {"n_wg", (int)p.wg_vtx.size()},
        {"n_split", (int)p.split_vtx.size()}, {"n_term", p.n_term}, {"wg_t512", p.wg_t512}, {"wg_lds_bytes", p.wg_lds_bytes},
        {"launch_lds_bytes", gcsadmm_k::wg_launch_lds_bytes(p.wg_lds_bytes, p.fused_tail != 0)},
        {"tail_lds_bytes", gcsadmm_k::FUSED_TAIL_LDS_BYTES}, {"edge_block", gcsadmm_k::EDGE_BLOCK},
    };
    for (const auto &f : fields)
        if (!std::strcmp(f.name, name)) return f.value;
    return -1;
}
