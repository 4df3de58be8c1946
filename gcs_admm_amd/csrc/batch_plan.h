// batch_plan.h -- what gcsadmm_batch_create decides before it allocates anything: which handles may share a set of launches, and the
// geometry of those launches.  Host-only and HIP-free like create_plan.h, whose plans are its input, so that the rules and the
// geometry can be tested on a machine without a GPU (tests/hostemu/batch_plan_emu.cpp, tests/test_batch_plan.py).
//
// A batch is a set of ordinary handles.  Its two kernels (vertex_wg_batch_kernel, edge_batch_kernel) pick the member by blockIdx.y and
// run the device functions of the solo kernels on that member's own arguments, so a member is eligible exactly when ONE launch of ONE
// instantiation of the in-LDS workgroup program does its whole vertex step, and one launch of the edge kernel its edge step.
// GCSADMM_BATCH_LARGE adds a third kernel, vertex_wave_batch_kernel, for members with vertices on the wavefront program: one launch per
// group of members that run the same instantiation of it (WaveGroup below), beside the workgroup launch of those that have one.
// GCSADMM_BATCH_TERMINALS adds terminal_region_batch_kernel for members with a terminal that is a region: one launch per group of
// terminals that run with the same thread count and keep their work arrays in the same place (TermGroup below).
#pragma once
#include <algorithm>
#include <string>
#include <vector>

#include "create_plan.h"

namespace gcsadmm_k {

constexpr int BATCH_MAX_MEMBERS = 65535;     // members are rows of the launch grid (gridDim.y)

// a member as the rules see it: the plan its create made, the descriptor's scalars and what its handle holds
struct BatchMember {
    const void *id;             // identity of the handle (a handle may appear once)
    const CreatePlan *plan;
    int n, dtype, device;
    int n_wg, n_special, n_split;       // vertices on the in-LDS workgroup program, closed-form vertices, split-form vertices
    int has_comm;               // a communicator / halo is attached (gcsadmm_attach_comm)
};

// one launch of vertex_wave_batch_kernel (GCSADMM_BATCH_LARGE): the members whose wavefront vertices run one instantiation
struct WaveGroup {
    int all_m4 = 0, align_rows = 0, store_dl = 0;      // the plan's three choices that select the instantiation (vertex_kernel.h)
    int grid_x = 0, lds_bytes = 0;                      // grid (grid_x, members.size()), 64 threads; dynamic LDS of the largest member
    std::vector<int> members;                           // indices into the batch, ascending
};

// one launch of terminal_region_batch_kernel (GCSADMM_BATCH_TERMINALS): the terminals -- not the members: a member may have two -- whose
// solves run with one thread count and one home of the work arrays.  The reductions of the solve depend on the thread count and the
// home is a template parameter of the kernel, so these two are what a terminal's solo launch and its batch launch must share.
struct TermGroup {
    int threads = 0, in_lds = 0;                        // 64 or 256 (plan.term_threads); plan.term_lds_doubles > 0
    int lds_doubles = 0;                                // dynamic LDS of the launch: the largest term_lds_doubles of the group's members
    std::vector<int> member, term;                      // entry k: terminal term[k] of member member[k]; by member, then by terminal
};

struct BatchPlan {
    int count = 0, n = 0, dtype = 0, device = 0, box = 0;
    // vertex launch: grid (vertex_grid_x, count), 256 threads, vertex_lds_bytes of dynamic LDS; member m uses the first vertex_grid[m] columns
    int vertex_grid_x = 0, vertex_lds_bytes = 0;
    // edge launch: grid (edge_grid_x, count), EDGE_BLOCK threads; member m uses the first edge_blocks[m] columns
    int edge_grid_x = 0;
    std::vector<int> vertex_grid, edge_blocks;
    // GCSADMM_BATCH_LARGE: the workgroup launch has a row for each of wg_members only (without the flag: every member, in order), and
    // the wavefront vertices run one launch per group; wave_grid[m]: wavefronts + closed-form workgroups of member m, 0: none
    unsigned flags = 0;
    std::vector<int> wg_members, wave_grid;
    std::vector<WaveGroup> wave_groups;
    // GCSADMM_BATCH_TERMINALS: the region terminals of all members, one launch per group, grid = entries of the group; at most four groups
    std::vector<TermGroup> term_groups;
};

// the eligibility rules, in the order they are checked, and the launch geometry; `err` names the member and the reason.
// flags = 0: one launch of the in-LDS workgroup program at 256 threads is every member's whole vertex step.  GCSADMM_BATCH_LARGE: a
// member may also have vertices on the wavefront program (n = 2) -- they run vertex_wave_batch_kernel, one launch per group of members
// that share (all_m4, align_rows, store_dl), and carry the member's closed-form vertices as launch_vertex does for a solo handle --
// and any number of workgroup-program vertices: a batch does no slowest-first reorder (that changes scheduling, never results).
// GCSADMM_BATCH_TERMINALS: a member may have terminals that are regions; they are listed in term_groups by (term_threads,
// term_lds_doubles > 0) of the member's create plan.  Without it the verdicts, the texts and the plan are what they were before the flag.
inline gcsadmm_status make_batch_plan(const BatchMember *m, int count, BatchPlan &bp, std::string &err, unsigned flags = 0)
{
    const bool large = (flags & GCSADMM_BATCH_LARGE) != 0;
    auto fail = [&](gcsadmm_status st, int i, const char *why) {
        err = i < 0 ? std::string(why) : "member " + std::to_string(i) + ": " + why;
        return st;
    };
    bp = BatchPlan();
    const bool terminals = (flags & GCSADMM_BATCH_TERMINALS) != 0;
    if (flags & ~(unsigned)(GCSADMM_BATCH_LARGE | GCSADMM_BATCH_TERMINALS)) return fail(GCSADMM_ERR_BAD_ARG, -1, "unknown batch flag");
    if (!m || count < 1) return fail(GCSADMM_ERR_BAD_ARG, -1, "a batch needs at least one member");
    if (count > BATCH_MAX_MEMBERS) return fail(GCSADMM_ERR_UNSUPPORTED, -1, "a batch holds at most 65535 members");
    for (int i = 0; i < count; ++i) {
        if (!m[i].id || !m[i].plan) return fail(GCSADMM_ERR_BAD_ARG, i, "null handle");
        for (int j = 0; j < i; ++j)
            if (m[j].id == m[i].id) return fail(GCSADMM_ERR_BAD_ARG, i, "the handle appears twice in the batch");
    }
    int first_wg = 0;      // (large) the first member with workgroup-program vertices: its BOX choice is the launch's
    while (large && first_wg < count - 1 && m[first_wg].n_wg == 0) ++first_wg;
    for (int i = 0; i < count; ++i) {
        const CreatePlan &p = *m[i].plan;
        // one kernel instantiation serves the launch
        if (m[i].device != m[0].device) return fail(GCSADMM_ERR_BAD_ARG, i, "members must be on the same device");
        if (m[i].n != m[0].n) return fail(GCSADMM_ERR_UNSUPPORTED, i, "members must share the space dimension n");
        if (m[i].dtype != m[0].dtype) return fail(GCSADMM_ERR_UNSUPPORTED, i, "members must share the state_dtype");
        // one launch of the in-LDS workgroup program at 256 threads is the member's whole vertex step
        if (!large && p.n_waves() > 0) return fail(GCSADMM_ERR_UNSUPPORTED, i, "vertices on the wavefront program (create the handle with vertex_program = 3)");
        if (p.wg_t512) return fail(GCSADMM_ERR_UNSUPPORTED, i, "the workgroup program runs with 512 threads (create the handle with vertex_program = 3)");
        if (m[i].n_split > 0) return fail(GCSADMM_ERR_UNSUPPORTED, i, "vertices in the split form of the workgroup program (vertex_workspace)");
        if (!terminals && p.n_term > 0) return fail(GCSADMM_ERR_UNSUPPORTED, i, "a terminal that is a region");
        if (!large && (p.wg_reorder || m[i].n_wg >= REORDER_MIN_UNITS)) return fail(GCSADMM_ERR_UNSUPPORTED, i, "512 or more workgroup-program vertices (slowest-first dispatch)");
        if (p.edge_unroll != 1) return fail(GCSADMM_ERR_UNSUPPORTED, i, "the edge step runs unrolled (a graph this large gains nothing from a batch)");
        if (m[i].has_comm) return fail(GCSADMM_ERR_UNSUPPORTED, i, "a communicator is attached (partitioned handles run their own loop)");
        // (large: among the members that have workgroup-program vertices; the closed-form workgroups are the same in both instantiations)
        if ((!large || m[i].n_wg > 0) && p.wg_box != m[first_wg].plan->wg_box)
            return fail(GCSADMM_ERR_UNSUPPORTED, i, "members must share the BOX choice of the workgroup program (plan.wg_box)");
    }
    bp.count = count; bp.n = m[0].n; bp.dtype = m[0].dtype; bp.device = m[0].device; bp.box = m[first_wg].plan->wg_box; bp.flags = flags;
    for (int i = 0; i < count; ++i) {
        const CreatePlan &p = *m[i].plan;
        // the closed-form vertices ride on the wave launch of a member that has one (launch_vertex's special_on_wave), else here
        const bool special_on_wave = large && p.n_waves() > 0;
        const int grid = m[i].n_wg + (special_on_wave ? 0 : (m[i].n_special + 255) / 256);
        bp.vertex_grid.push_back(grid);
        bp.edge_blocks.push_back(p.edge_blocks);
        bp.edge_grid_x = std::max(bp.edge_grid_x, p.edge_blocks);
        bp.wave_grid.push_back(special_on_wave ? p.n_waves() + (m[i].n_special + 63) / 64 : 0);
        if (!large || grid > 0) {
            bp.wg_members.push_back(i);
            bp.vertex_grid_x = std::max(bp.vertex_grid_x, grid);
            bp.vertex_lds_bytes = std::max(bp.vertex_lds_bytes, std::max(p.wg_lds_bytes, 4 * MAX_SPECIAL_DEG * 8));
        }
        for (int ti = 0; ti < p.n_term; ++ti) {
            const int in_lds = p.term_lds_doubles > 0;
            auto g = std::find_if(bp.term_groups.begin(), bp.term_groups.end(),
                                  [&](const TermGroup &t) { return t.threads == p.term_threads && t.in_lds == in_lds; });
            if (g == bp.term_groups.end()) {
                bp.term_groups.push_back(TermGroup{p.term_threads, in_lds});
                g = bp.term_groups.end() - 1;
            }
            g->member.push_back(i); g->term.push_back(ti);
            g->lds_doubles = std::max(g->lds_doubles, p.term_lds_doubles);
        }
        if (!special_on_wave) continue;
        auto g = std::find_if(bp.wave_groups.begin(), bp.wave_groups.end(),
                              [&](const WaveGroup &w) { return w.all_m4 == p.all_m4 && w.align_rows == p.align_rows && w.store_dl == p.store_dl; });
        if (g == bp.wave_groups.end()) {
            bp.wave_groups.push_back(WaveGroup{p.all_m4, p.align_rows, p.store_dl});
            g = bp.wave_groups.end() - 1;
        }
        g->members.push_back(i);
        g->grid_x = std::max(g->grid_x, bp.wave_grid.back());
        g->lds_bytes = std::max(g->lds_bytes, std::max(p.lds_bytes, 4 * MAX_SPECIAL_DEG * 8));
    }
    return GCSADMM_OK;
}

}  // namespace gcsadmm_k
