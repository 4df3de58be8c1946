// batch_terminals_plan_emu.cpp -- gcsadmm_batch_create_ex's decisions under GCSADMM_BATCH_TERMINALS (gcs_admm_amd/csrc/batch_plan.h) on
// the host, for tests/test_batch_terminals_plan.py: members are made from descriptors as gcsadmm_create makes its plans
// (create_plan.h), then the batch rules run with the caller's flags and the terminal groups are read back by name.  Linked with
// wg_sizes.cpp built at 256 and at 512 threads, as batch_plan_emu.cpp is.  Test-only; the product has no path into it.
#include <cmath>
#include <cstring>
#include <memory>

#include "batch_plan.h"
#include "terminal_region.h"

long long gcsadmm_terminal_ws_doubles(int n, int facets, int live_edges) { return gcs_term::terminal_ws_doubles(n, facets, live_edges); }
long long gcsadmm_terminal_record_doubles(int n, int facets, int live_edges) { return gcs_term::terminal_record_doubles(n, facets, live_edges); }

using namespace gcsadmm_k;

struct Member {
    CreatePlan plan;
    int n, dtype, device, has_comm;
};
static std::vector<std::unique_ptr<Member>> g_members;
static BatchPlan g_batch;
static std::string g_err;

extern "C" void term_emu_clear() { g_members.clear(); g_err.clear(); }

// a handle as gcsadmm_create would make it (a device is taken to be present); returns its index, or -1 - status where create refuses
extern "C" int term_emu_add(const gcsadmm_graph_desc *g, int has_comm)
{
    auto m = std::make_unique<Member>();
    gcsadmm_status st = check_graph_desc(g, g_err);
    if (st == GCSADMM_OK) st = make_create_plan(*g, m->plan, g_err);
    if (st != GCSADMM_OK) return -1 - (int)st;
    m->n = g->n; m->dtype = g->state_dtype; m->device = g->device; m->has_comm = has_comm;
    g_members.push_back(std::move(m));
    return (int)g_members.size() - 1;
}

// status of make_batch_plan(.., flags) over the members idx[0 .. count); the message: term_emu_error
extern "C" int term_emu_make(const int *idx, int count, unsigned flags)
{
    std::vector<BatchMember> ms;
    for (int i = 0; i < count; ++i) {
        const Member &m = *g_members[idx[i]];
        ms.push_back(BatchMember{&m, &m.plan, m.n, m.dtype, m.device, (int)m.plan.wg_vtx.size(), (int)m.plan.special_vtx.size(),
                                 (int)m.plan.split_vtx.size(), m.has_comm});
    }
    g_err.clear();
    return (int)make_batch_plan(ms.data(), count, g_batch, g_err, flags);
}

extern "C" const char *term_emu_error() { return g_err.c_str(); }

// scalar field of the last batch plan; NaN: no such field
extern "C" double term_emu_get(const char *name)
{
    const BatchPlan &b = g_batch;
    const struct { const char *name; double value; } fields[] = {
        {"count", (double)b.count}, {"n", (double)b.n}, {"dtype", (double)b.dtype}, {"device", (double)b.device}, {"box", (double)b.box},
        {"vertex_grid_x", (double)b.vertex_grid_x}, {"vertex_lds_bytes", (double)b.vertex_lds_bytes}, {"edge_grid_x", (double)b.edge_grid_x},
        {"flags", (double)b.flags}, {"wg_members", (double)b.wg_members.size()}, {"wave_groups", (double)b.wave_groups.size()},
        {"term_groups", (double)b.term_groups.size()},
    };
    for (const auto &f : fields)
        if (!std::strcmp(f.name, name)) return f.value;
    return NAN;
}

// per-member field of the last batch plan: "vertex_grid", "edge_blocks", "wave_grid" of member `at`
extern "C" double term_emu_member(const char *name, int at)
{
    if (!std::strcmp(name, "vertex_grid")) return (double)g_batch.vertex_grid[at];
    if (!std::strcmp(name, "edge_blocks")) return (double)g_batch.edge_blocks[at];
    if (!std::strcmp(name, "wave_grid")) return (double)g_batch.wave_grid[at];
    return NAN;
}

// field of terminal group `group` of the last batch plan: "threads", "in_lds", "lds_doubles", "entries" (how many), "member" / "term":
// the member and its terminal in entry `at` of the group's table
extern "C" double term_emu_group(const char *name, int group, int at)
{
    const TermGroup &g = g_batch.term_groups[group];
    if (!std::strcmp(name, "threads")) return (double)g.threads;
    if (!std::strcmp(name, "in_lds")) return (double)g.in_lds;
    if (!std::strcmp(name, "lds_doubles")) return (double)g.lds_doubles;
    if (!std::strcmp(name, "entries")) return (double)g.member.size();
    if (!std::strcmp(name, "member")) return (double)g.member[at];
    if (!std::strcmp(name, "term")) return (double)g.term[at];
    return NAN;
}
