// vertex_wg_launch.h -- host-side interface of the workgroup-cooperative vertex kernel (vertex_wg.hip), used by
// gcsadmm.hip.  Plain pointers (device) and scalars; one object file per program keeps the builds parallel.
#pragma once
#include <hip/hip_runtime.h>

#include "edge_step.h"
#include "gcsadmm.h"
#include "step_args.h"

namespace gcsadmm_k {

// FUSED TAIL of an in-LDS launch (vertex_wg_kernel.h): what the last workgroup to finish needs to run the single-workgroup edge step and
// the control step -- the arguments edge_kernel MODE 1 gets (state untyped, as in StepDesc) and the handle's arrival counter.
// enabled = 0 (every launch but gcsadmm_run's on a handle whose plan has fused_tail): the launch is the vertex step alone.
struct WgTailDesc {
    int enabled = 0;
    EdgeArgs<void> edge{};
    gcsadmm_control_block *cb = nullptr;      // writable: the control step's
    double *sums = nullptr;
    ControlParams cp{};
    int *counters = nullptr;
    double *trace = nullptr;                  // may be null
    unsigned *ticket = nullptr;
};

struct WgLaunchDesc {
    StepDesc step;
    int n, dtype;                   // space dimension 1 .. 8, GCSADMM_F64 / GCSADMM_F32
    int n_vtx, n_special, lds_bytes;
    const int *vtx;                 // [n_vtx] generic vertices of this launch, one workgroup each
    const int *special_vtx, *special_kind;   // trailing workgroups (may be empty: n_special = 0)
    int box;                        // every vertex of the launch is a canonical axis-aligned box (canonical_box.h): BOX instantiation
    const int *order;               // slowest-first dispatch (reorder_kernel): workgroup b solves vtx[order[b]]; may be null
    int *unit_iters;                // [n_vtx] Newton iterations of each vertex's last solve; may be null
    WgTailDesc tail;                // in-LDS launch only
};

// the split form's device-memory workspace: the units of vtx[b] of the launch at units + unit_off[b] (256-byte aligned slabs)
struct WgSplitArgs {
    double *units;
    const long long *unit_off;      // [n_vtx] offsets in doubles
};

// one vertex-step launch for a batch of handles (vertex_wg_batch_kernel; 256-thread objects only): `table` is a device array of `count`
// entries, one per member, laid out by gcsadmm_wg_batch_fill
struct WgBatchLaunch {
    int n, dtype, box;              // shared by the members: one kernel instantiation serves the launch
    const void *table;
    unsigned grid_x, count;         // workgroups of the widest member, members
    int lds_bytes;                  // dynamic LDS of the largest member
};

}  // namespace gcsadmm_k

// (LDS sizes of the program, gcsadmm_wg_lds_bytes / _t512 and gcsadmm_wg_has_box: create_plan.h, which is host-only)
// raise the dynamic-LDS limit of the instantiation (needed above 48 KB)
hipError_t gcsadmm_wg_set_lds(int n, int dtype, int lds_bytes);
void gcsadmm_wg_launch(const gcsadmm_k::WgLaunchDesc &d, hipStream_t s);

// the same program built with 512 threads per workgroup (second objects of vertex_wg.hip and vertex_wg_dims.hip): 3-10 % faster while every
// workgroup has a CU to itself (benchmark3 5 656 -> 6 244 it/s, benchmark4 7 590 -> 7 955), slower beyond (1 026 vertices: 5 763 -> 3 932)
hipError_t gcsadmm_wg_set_lds_t512(int n, int dtype, int lds_bytes);
void gcsadmm_wg_launch_t512(const gcsadmm_k::WgLaunchDesc &d, hipStream_t s);

// the split form (vertex_wg_split_kernel; 256-thread objects only): d.vtx / d.n_vtx are the split vertices, d.lds_bytes the LDS of the
// fixed block and the polytope (at least 48 KB needs the attribute below), d.box as for the in-LDS launch; d.n_special, d.order and
// d.unit_iters are unused
hipError_t gcsadmm_wg_set_split_lds(int n, int dtype, int lds_bytes);
void gcsadmm_wg_launch_split(const gcsadmm_k::WgLaunchDesc &d, const gcsadmm_k::WgSplitArgs &w, hipStream_t s);

// the batch form: bytes of one table entry for that state type; fill the entry at `entry_host` from the member's in-LDS launch (d.step.cb
// is the member's control block; the entry records the width of the member's own grid and returns it); raise the batch kernels' dynamic-LDS
// limit; launch
size_t gcsadmm_wg_batch_entry_bytes(int dtype);
int gcsadmm_wg_batch_fill(const gcsadmm_k::WgLaunchDesc &d, void *entry_host);
hipError_t gcsadmm_wg_set_batch_lds(int n, int dtype, int lds_bytes);
void gcsadmm_wg_launch_batch(const gcsadmm_k::WgBatchLaunch &b, hipStream_t s);

// PROX configuration of the workgroup program (gcsadmm_vertex_prox): every vertex of `vtx` solves the border-only problem with
// the separable quadratic (q, c) [V][4n+1]; the two terminals (points) are closed form.  zedge / mu / copy of `d` are unused.
void gcsadmm_wg_launch_prox(const gcsadmm_k::WgLaunchDesc &d, const double *q, const double *c, int src, int dst, hipStream_t s);
