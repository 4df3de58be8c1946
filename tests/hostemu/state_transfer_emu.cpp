// Host build of the state-transfer kernels (csrc/state_transfer_core.h): the checks and the table of gcsadmm_export_state /
// gcsadmm_import_state and their batch forms as gcsadmm.hip makes them (transfer_add on every member with a snapshot), then every lane
// of every workgroup of the one launch run one after the other -- forwards or backwards -- on host arrays.
// Test infrastructure: never shipped, never timed.
#include <string>
#include <vector>
#include "state_transfer_core.h"
using namespace gcsadmm_k;

namespace {

// what a handle is to the transfer: the descriptor's sizes, both ends and both columns of every edge, the control block
struct Handle {
    TransferHandle h{};
    std::vector<int> tail, head, inc_tail, inc_head;
    gcsadmm_control_block cb{};
};
std::string g_err;

template <class T> void run(const TransferCall &call, bool exporting, bool backwards)
{
    const int count = (int)call.table.size();
    for (int b = 0; b < call.blocks; ++b) {
        const int block = backwards ? call.blocks - 1 - b : b;
        const TransferEntry e = call.table[(size_t)transfer_member(call.table.data(), count, block)];      // the kernel's first line
        for (int l = 0; l < TRANSFER_BLOCK; ++l) {
            const int lane = backwards ? TRANSFER_BLOCK - 1 - l : l;
            if (exporting) transfer_export_lane<T>(e, block - e.block_first, lane);
            else transfer_import_lane<T>(e, block - e.block_first, lane);
        }
    }
}

}  // namespace

extern "C" {

void *ste_create(int n, int dtype, int V, int E, int NI, int edge_major, const int *edge_tail, const int *edge_head, const int *inc_tail, const int *inc_head)
{
    Handle *p = new Handle();
    p->tail.assign(edge_tail, edge_tail + E); p->head.assign(edge_head, edge_head + E);
    p->inc_tail.assign(inc_tail, inc_tail + E); p->inc_head.assign(inc_head, inc_head + E);
    p->h = TransferHandle{n, dtype, V, E, NI, edge_major, transfer_edges_ascend(E, p->tail.data(), p->head.data()), false,
                          p->tail.data(), p->head.data(), p->inc_tail.data(), p->inc_head.data(), &p->cb};
    return p;
}
void ste_destroy(void *h) { delete (Handle *)h; }
// gcsadmm_reset, and what a run leaves behind: rho and a pending rescale
void ste_reset(void *h, double rho, double mu_scale)
{
    Handle *p = (Handle *)h;
    p->cb.rho = rho; p->cb.mu_scale = mu_scale; p->h.reset = true;
}
const char *ste_last_error(void) { return g_err.c_str(); }

// solo != 0: gcsadmm_export_state / gcsadmm_import_state on handles[0]; otherwise the batch forms over `count` members, a null
// snapshots[i] skipping member i
int ste_transfer(int count, void *const *handles, const gcsadmm_state *states, const int32_t *const *vertex_ids, gcsadmm_snapshot *const *snapshots,
                 int exporting, int solo, int backwards)
{
    TransferCall call;
    if (!solo && (!vertex_ids || !snapshots)) { g_err = "null vertex_ids or snapshots"; return GCSADMM_ERR_BAD_ARG; }
    for (int i = 0; i < count; ++i) {
        if (!solo && !snapshots[i]) continue;
        const Handle *p = (const Handle *)handles[i];
        const gcsadmm_status st = transfer_add(call, p->h, &states[i], vertex_ids ? vertex_ids[i] : nullptr, snapshots ? snapshots[i] : nullptr, exporting != 0,
                                               solo ? std::string() : "member " + std::to_string(i) + ": ", g_err);
        if (st != GCSADMM_OK) return st;
    }
    for (size_t i = 0; i < call.table.size(); ++i) call.table[i].vertex_id = call.ids.data() + call.ids_at[i];
    const int dtype = call.table.empty() ? GCSADMM_F64 : ((const Handle *)handles[0])->h.dtype;
    if (dtype == GCSADMM_F64) run<double>(call, exporting != 0, backwards != 0);
    else run<float>(call, exporting != 0, backwards != 0);
    for (int i = 0; exporting && i < count; ++i)
        if (solo || snapshots[i]) { snapshots[i]->V = ((const Handle *)handles[i])->h.V; snapshots[i]->E = ((const Handle *)handles[i])->h.E; }
    return GCSADMM_OK;
}

}  // extern "C"
