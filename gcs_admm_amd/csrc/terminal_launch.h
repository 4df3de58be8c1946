// terminal_launch.h -- host-side interface of the region-terminal kernel (terminal_region.hip), used by gcsadmm.hip.
#pragma once
#include <hip/hip_runtime.h>

#include "gcsadmm.h"
#include "step_args.h"

namespace gcsadmm_k {

// what the kernel takes besides StepArgs: the terminals of the launch and their work arrays
struct TermBlock {
    int vtx[2], is_src[2];
    double *ws;                     // workspace of each terminal, ws + ws_off[i], gcsadmm_terminal_ws_doubles(n, facets, live edges) doubles
    long long ws_off[2];
    double *rec;                    // warm-start records (terminal_region.h), rec + rec_off[i]; nullptr: every solve starts cold
    long long rec_off[2];
};

struct TermLaunchDesc {
    StepDesc step;
    TermBlock t;
    int n, dtype;                   // space dimension 1 .. 8, GCSADMM_F64 / GCSADMM_F32
    int count;                      // region terminals of the handle: 0, 1 or 2 -- one workgroup each
    int threads;                    // 64 (one wavefront: small terminals) or 256
    int lds_doubles;                // > 0: the work arrays of every terminal fit this much dynamic LDS and live there; 0: in ws
};

// entry of the table of terminal_region_batch_kernel: what the solo kernel of the terminal's handle gets as arguments, and which of
// the handle's terminals the workgroup solves
template <class T> struct TermBatchEntry {
    StepArgs<T> a;
    TermBlock t;
    const gcsadmm_control_block *cb;
    int ti;
};

// one terminal launch of a batch: `table` is a device array of `count` entries laid out by gcsadmm_terminal_batch_fill, one per
// terminal of the group; every terminal of the group runs with `threads` threads and keeps its work arrays in LDS or not as the group does
struct TermBatchLaunch {
    int n, dtype;
    const void *table;
    int count, threads;
    int lds_doubles;                // the largest of the group's members; 0: the group's terminals work in their handles' ws
};

}  // namespace gcsadmm_k

// (work-array and record sizes, gcsadmm_terminal_ws_doubles / gcsadmm_terminal_record_doubles: create_plan.h, which is host-only)
void gcsadmm_terminal_launch(const gcsadmm_k::TermLaunchDesc &d, hipStream_t s);
// the batch form: bytes of a table entry for that state type; the entry of terminal `ti` of the handle whose solo launch is `d`; the launch
size_t gcsadmm_terminal_batch_entry_bytes(int dtype);
void gcsadmm_terminal_batch_fill(const gcsadmm_k::TermLaunchDesc &d, int ti, void *entry_host);
void gcsadmm_terminal_launch_batch(const gcsadmm_k::TermBatchLaunch &b, hipStream_t s);
