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

}  // namespace gcsadmm_k

// (work-array and record sizes, gcsadmm_terminal_ws_doubles / gcsadmm_terminal_record_doubles: create_plan.h, which is host-only)
void gcsadmm_terminal_launch(const gcsadmm_k::TermLaunchDesc &d, hipStream_t s);
