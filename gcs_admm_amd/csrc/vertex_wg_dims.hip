// vertex_wg_dims.hip -- the workgroup-cooperative vertex program (vertex_wg.h, vertex_wg_kernel.h) instantiated for the space
// dimensions BASELINE.json does not name: n = 1, 4, 5, 7, 8 (7: the configuration space of a seven-joint arm).  The reference's sub-problem takes
// any n (admm_solver_v3.py:363-377); the program is the same template.  Generic instantiation only (the BOX one exists for the tuned dimensions 3 and 6).
// Built twice like vertex_wg.hip (256 / 512 threads per workgroup: gcs_admm_amd/build.py).
#include "vertex_wg_kernel.h"

using namespace gcsadmm_k;

#ifndef GCS_WG_SYM
#define GCS_WG_SYM(name) name
#endif

hipError_t GCS_WG_SYM(gcsadmm_wg_set_lds_dims)(int n, int dtype, int lds_bytes)
{
    hipError_t e = hipErrorInvalidValue;
    dispatch_dim<1, 4, 5, 7, 8>(n, [&](auto nn) { e = set_lds<InLdsKernels, decltype(nn)::value>(dtype, lds_bytes); });
    return e;
}

void GCS_WG_SYM(gcsadmm_wg_launch_dims)(const WgLaunchDesc &d, hipStream_t s)
{
    dispatch_dim<1, 4, 5, 7, 8>(d.n, [&](auto nn) { launch<decltype(nn)::value>(d, s); });
}

void GCS_WG_SYM(gcsadmm_wg_launch_prox_dims)(const WgLaunchDesc &d, const double *q, const double *c, int src, int dst, hipStream_t s)
{
    dispatch_dim<1, 4, 5, 7, 8>(d.n, [&](auto nn) { launch_prox<decltype(nn)::value>(d, q, c, src, dst, s); });
}

#if GCS_WG_THREADS == 256
hipError_t gcsadmm_wg_set_split_lds_dims(int n, int dtype, int lds_bytes)
{
    hipError_t e = hipErrorInvalidValue;
    dispatch_dim<1, 4, 5, 7, 8>(n, [&](auto nn) { e = set_lds<SplitKernels, decltype(nn)::value>(dtype, lds_bytes); });
    return e;
}

void gcsadmm_wg_launch_split_dims(const WgLaunchDesc &d, const WgSplitArgs &w, hipStream_t s)
{
    dispatch_dim<1, 4, 5, 7, 8>(d.n, [&](auto nn) { launch_split<decltype(nn)::value>(d, w, s); });
}

hipError_t gcsadmm_wg_set_batch_lds_dims(int n, int dtype, int lds_bytes)
{
    hipError_t e = hipErrorInvalidValue;
    dispatch_dim<1, 4, 5, 7, 8>(n, [&](auto nn) { e = set_lds<BatchKernels, decltype(nn)::value>(dtype, lds_bytes); });
    return e;
}

void gcsadmm_wg_launch_batch_dims(const WgBatchLaunch &b, hipStream_t s)
{
    dispatch_dim<1, 4, 5, 7, 8>(b.n, [&](auto nn) { launch_batch<decltype(nn)::value>(b, s); });
}
#endif
