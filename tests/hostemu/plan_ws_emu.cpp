// plan_ws_emu.cpp -- the plan shim of tests/test_create_plan.py (plan_emu.cpp, included whole) plus the fields of the split form of
// the workgroup program (gcsadmm_graph_desc.vertex_workspace), for tests/test_vertex_workspace_plan.py.  Test-only.
#include "plan_emu.cpp"
#include "vertex_wg.h"

// split_vtx / split_off of the last plan: their length (the first `cap` entries go to `out`); -1: no such field
extern "C" long long plan_ws_emu_vec(const char *name, double *out, long long cap)
{
    if (!std::strcmp(name, "split_vtx")) return copy_out(g_plan.split_vtx, out, cap);
    if (!std::strcmp(name, "split_off")) return copy_out(g_plan.split_off, out, cap);
    return -1;
}

// scalar fields: split_doubles, split_lds_bytes; NaN otherwise
extern "C" double plan_ws_emu_get(const char *name)
{
    if (!std::strcmp(name, "split_doubles")) return (double)g_plan.split_doubles;
    if (!std::strcmp(name, "split_lds_bytes")) return (double)g_plan.split_lds_bytes;
    return NAN;
}

// the split layout of the 256-thread build: LDS doubles of the fixed block and the polytope
extern "C" int plan_ws_emu_split_lds_doubles(int n, int facets, int box) { return gcs_wg::wg_lds_doubles_n(n, 0, facets, box != 0); }
