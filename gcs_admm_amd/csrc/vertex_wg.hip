// vertex_wg.hip -- gfx950 kernel of the workgroup-cooperative vertex program (vertex_wg.h): one 256-thread workgroup
// per generic vertex, any degree and facet count that fits the CU's 160 KB of LDS.  Trailing workgroups of the launch take the
// closed-form vertices (special_vertex.h).  This object instantiates the program for n = 2, 3, 6 and dispatches; n = 1, 4, 5, 7, 8 are in
// vertex_wg_dims.hip (same templates, vertex_wg_kernel.h).
// Replaces admm_solver_v3.py:469-540 (one MOSEK solve per vertex through SolveInParallel) for the vertices routed here
// by gcsadmm_create: small graphs, n != 2, degree > 63.
// The object is built twice (gcs_admm_amd/build.py): with 256 threads per workgroup, and with 512 for launches of at most one workgroup
// per CU (-DGCS_WG_THREADS=512 -Dgcs_wg=gcs_wg_t512 -D'GCS_WG_SYM(name)=name##_t512': own namespace, own entry points; gcsadmm.hip
// chooses at create).
#include "vertex_wg_kernel.h"

using namespace gcsadmm_k;

#ifndef GCS_WG_SYM
#define GCS_WG_SYM(name) name
#endif

// n = 1, 4, 5, 7, 8 (vertex_wg_dims.hip, the object of the same thread count)
hipError_t GCS_WG_SYM(gcsadmm_wg_set_lds_dims)(int n, int dtype, int lds_bytes);
void GCS_WG_SYM(gcsadmm_wg_launch_dims)(const WgLaunchDesc &d, hipStream_t s);
void GCS_WG_SYM(gcsadmm_wg_launch_prox_dims)(const WgLaunchDesc &d, const double *q, const double *c, int src, int dst, hipStream_t s);


int GCS_WG_SYM(gcsadmm_wg_lds_bytes)(int n, int units, int facets, bool box) { return 8 * gcs_wg::wg_lds_doubles_n(n, units, facets, box); }
bool GCS_WG_SYM(gcsadmm_wg_has_box)(int n) { return gcs_wg::wg_has_box(n); }

hipError_t GCS_WG_SYM(gcsadmm_wg_set_lds)(int n, int dtype, int lds_bytes)
{
    hipError_t e = hipSuccess;
    if (dispatch_dim<2, 3, 6>(n, [&](auto nn) { e = set_lds<InLdsKernels, decltype(nn)::value>(dtype, lds_bytes); })) return e;
    return GCS_WG_SYM(gcsadmm_wg_set_lds_dims)(n, dtype, lds_bytes);
}

void GCS_WG_SYM(gcsadmm_wg_launch)(const WgLaunchDesc &d, hipStream_t s)
{
    if (!dispatch_dim<2, 3, 6>(d.n, [&](auto nn) { launch<decltype(nn)::value>(d, s); })) GCS_WG_SYM(gcsadmm_wg_launch_dims)(d, s);
}

void GCS_WG_SYM(gcsadmm_wg_launch_prox)(const WgLaunchDesc &d, const double *q, const double *c, int src, int dst, hipStream_t s)
{
    if (!dispatch_dim<2, 3, 6>(d.n, [&](auto nn) { launch_prox<decltype(nn)::value>(d, q, c, src, dst, s); }))
        GCS_WG_SYM(gcsadmm_wg_launch_prox_dims)(d, q, c, src, dst, s);
}

#if GCS_WG_THREADS == 256
// the split form (units in device memory), 256-thread build only
hipError_t gcsadmm_wg_set_split_lds_dims(int n, int dtype, int lds_bytes);
void gcsadmm_wg_launch_split_dims(const WgLaunchDesc &d, const WgSplitArgs &w, hipStream_t s);

hipError_t gcsadmm_wg_set_split_lds(int n, int dtype, int lds_bytes)
{
    hipError_t e = hipSuccess;
    if (dispatch_dim<2, 3, 6>(n, [&](auto nn) { e = set_lds<SplitKernels, decltype(nn)::value>(dtype, lds_bytes); })) return e;
    return gcsadmm_wg_set_split_lds_dims(n, dtype, lds_bytes);
}

void gcsadmm_wg_launch_split(const WgLaunchDesc &d, const WgSplitArgs &w, hipStream_t s)
{
    if (!dispatch_dim<2, 3, 6>(d.n, [&](auto nn) { launch_split<decltype(nn)::value>(d, w, s); })) gcsadmm_wg_launch_split_dims(d, w, s);
}

// the batch form (one launch for many handles), 256-thread build only
hipError_t gcsadmm_wg_set_batch_lds_dims(int n, int dtype, int lds_bytes);
void gcsadmm_wg_launch_batch_dims(const WgBatchLaunch &b, hipStream_t s);

size_t gcsadmm_wg_batch_entry_bytes(int dtype) { return dtype == GCSADMM_F64 ? sizeof(WgBatchEntry<double>) : sizeof(WgBatchEntry<float>); }

int gcsadmm_wg_batch_fill(const WgLaunchDesc &d, void *entry_host)
{
    const int grid_x = d.n_vtx + (d.n_special + WG_THREADS - 1) / WG_THREADS;
    with_state(d.dtype, [&](auto t) {
        using T = decltype(t);
        *(WgBatchEntry<T> *)entry_host = WgBatchEntry<T>{in_lds_args<T>(d), SpecialArgs{d.n_special, d.special_vtx, d.special_kind}, d.step.cb, grid_x};
    });
    return grid_x;
}

hipError_t gcsadmm_wg_set_batch_lds(int n, int dtype, int lds_bytes)
{
    hipError_t e = hipSuccess;
    if (dispatch_dim<2, 3, 6>(n, [&](auto nn) { e = set_lds<BatchKernels, decltype(nn)::value>(dtype, lds_bytes); })) return e;
    return gcsadmm_wg_set_batch_lds_dims(n, dtype, lds_bytes);
}

void gcsadmm_wg_launch_batch(const WgBatchLaunch &b, hipStream_t s)
{
    if (!dispatch_dim<2, 3, 6>(b.n, [&](auto nn) { launch_batch<decltype(nn)::value>(b, s); })) gcsadmm_wg_launch_batch_dims(b, s);
}
#endif

#ifdef GCS_WG_TIMING
extern "C" int gcsadmm_debug_wg_cycles(unsigned long long *cycles64, unsigned long long *counts64)
{
    int e = (int)hipMemcpyFromSymbol(cycles64, HIP_SYMBOL(gcs_wg::g_wg_cycles), 64 * sizeof(unsigned long long));
    if (e == 0) e = (int)hipMemcpyFromSymbol(counts64, HIP_SYMBOL(gcs_wg::g_wg_counts), 64 * sizeof(unsigned long long));
    return e;
}
extern "C" int gcsadmm_debug_wg_wave_cycles(unsigned long long *cycles512)
{
    return (int)hipMemcpyFromSymbol(cycles512, HIP_SYMBOL(gcs_wg::g_wg_wave_cycles), 512 * sizeof(unsigned long long));
}
#endif
#ifdef GCS_WG_BLOCKTIME
extern "C" int gcsadmm_debug_wg_blocks(unsigned long long *ticks64, unsigned long long *iters64)
{
    int e = (int)hipMemcpyFromSymbol(ticks64, HIP_SYMBOL(g_wg_block_ticks), 64 * sizeof(unsigned long long));
    if (e == 0) e = (int)hipMemcpyFromSymbol(iters64, HIP_SYMBOL(g_wg_block_iters), 64 * sizeof(unsigned long long));
    return e;
}
#endif
