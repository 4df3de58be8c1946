// plan_emu.cpp -- gcsadmm_create's decisions (gcs_admm_amd/csrc/create_plan.h) on the host, for tests/test_create_plan.py: the
// checks create makes before and after it looks for a device, and every field of the plan, read back by name.  Linked with
// wg_sizes.cpp built at 256 and at 512 threads.  Test-only; the product has no path into it.
#include <cstring>

#include "create_plan.h"
#include "terminal_region.h"

long long gcsadmm_terminal_ws_doubles(int n, int facets, int live_edges) { return gcs_term::terminal_ws_doubles(n, facets, live_edges); }
long long gcsadmm_terminal_record_doubles(int n, int facets, int live_edges) { return gcs_term::terminal_record_doubles(n, facets, live_edges); }

static gcsadmm_k::CreatePlan g_plan;
static std::string g_err;

// status of check_graph_desc, then of make_create_plan (a device is taken to be present); the message: plan_emu_error
extern "C" int plan_emu_make(const gcsadmm_graph_desc *g)
{
    g_err.clear();
    gcsadmm_status st = gcsadmm_k::check_graph_desc(g, g_err);
    if (st == GCSADMM_OK) st = gcsadmm_k::make_create_plan(*g, g_plan, g_err);
    return (int)st;
}

extern "C" const char *plan_emu_error() { return g_err.c_str(); }

// scalar field of the last plan; NaN: no such field
extern "C" double plan_emu_get(const char *name)
{
    const gcsadmm_k::CreatePlan &p = g_plan;
    const struct { const char *name; double value; } fields[] = {
        {"n_term", (double)p.n_term}, {"term_vtx0", (double)p.term_vtx[0]}, {"term_vtx1", (double)p.term_vtx[1]},
        {"term_is_src0", (double)p.term_is_src[0]}, {"term_is_src1", (double)p.term_is_src[1]},
        {"term_ws_off0", (double)p.term_ws_off[0]}, {"term_ws_off1", (double)p.term_ws_off[1]},
        {"term_rec_off0", (double)p.term_rec_off[0]}, {"term_rec_off1", (double)p.term_rec_off[1]},
        {"term_ws_doubles", (double)p.term_ws_doubles}, {"term_rec_doubles", (double)p.term_rec_doubles},
        {"term_threads", (double)p.term_threads}, {"term_lds_doubles", (double)p.term_lds_doubles},
        {"wg_lds_bytes", (double)p.wg_lds_bytes}, {"wg_box", (double)p.wg_box}, {"wg_t512", (double)p.wg_t512},
        {"n_waves", (double)p.n_waves()}, {"slots_cap", (double)p.slots_cap}, {"align_rows", (double)p.align_rows},
        {"store_dl", (double)p.store_dl}, {"all_m4", (double)p.all_m4}, {"wave_mm", (double)p.wave_mm}, {"lds_bytes", (double)p.lds_bytes},
        {"wave_reorder", (double)p.wave_reorder}, {"wg_reorder", (double)p.wg_reorder}, {"prox_lds_bytes", (double)p.prox_lds_bytes},
        {"nx", p.nx}, {"nmu", p.nmu}, {"edge_unroll", (double)p.edge_unroll}, {"edge_blocks", (double)p.edge_blocks},
    };
    for (const auto &f : fields)
        if (!std::strcmp(f.name, name)) return f.value;
    return NAN;
}

template <class V> static long long copy_out(const V &v, double *out, long long cap)
{
    for (long long i = 0; i < (long long)v.size() && i < cap; ++i) out[i] = (double)v[i];
    return (long long)v.size();
}

// array field of the last plan: its length (the first `cap` entries are written to `out`); -1: no such field
extern "C" long long plan_emu_vec(const char *name, double *out, long long cap)
{
    const gcsadmm_k::CreatePlan &p = g_plan;
    if (!std::strcmp(name, "deg_in")) return copy_out(p.deg_in, out, cap);
    if (!std::strcmp(name, "bc")) return copy_out(p.bc, out, cap);
    if (!std::strcmp(name, "special_vtx")) return copy_out(p.special_vtx, out, cap);
    if (!std::strcmp(name, "special_kind")) return copy_out(p.special_kind, out, cap);
    if (!std::strcmp(name, "wg_vtx")) return copy_out(p.wg_vtx, out, cap);
    if (!std::strcmp(name, "wave_slot_ptr")) return copy_out(p.wave_slot_ptr, out, cap);
    if (!std::strcmp(name, "wave_vtx")) return copy_out(p.wave_vtx, out, cap);
    if (!std::strcmp(name, "warm_ptr")) return copy_out(p.warm_ptr, out, cap);
    if (!std::strcmp(name, "prox_vtx")) return copy_out(p.prox_vtx, out, cap);
    if (!std::strcmp(name, "col_owned")) return copy_out(p.col_owned, out, cap);
    if (!std::strcmp(name, "col_vertex")) return copy_out(p.col_vertex, out, cap);
    return -1;
}

// the sizing functions the plan calls, for the test's consistency checks
extern "C" int plan_emu_wg_lds_bytes(int t512, int n, int units, int facets, int box)
{
    return t512 ? gcsadmm_wg_lds_bytes_t512(n, units, facets, box != 0) : gcsadmm_wg_lds_bytes(n, units, facets, box != 0);
}
extern "C" long long plan_emu_term_ws_doubles(int n, int facets, int live) { return gcsadmm_terminal_ws_doubles(n, facets, live); }
extern "C" long long plan_emu_term_record_doubles(int n, int facets, int live) { return gcsadmm_terminal_record_doubles(n, facets, live); }
extern "C" long long plan_emu_warm_record_doubles(int n, int facets, int degree) { return gcs_ws::warm_record_doubles(n, facets, degree); }
