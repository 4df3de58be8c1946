// vertex_wg_kernel.h -- the kernel templates of the workgroup-cooperative vertex program and their launch helpers, shared by the two
// translation units that instantiate them: vertex_wg.hip (n = 2, 3, 6: the dimensions of BASELINE.json's configs) and
// vertex_wg_dims.hip (n = 1, 4, 5, 7, 8: the program is dimension-generic, as the reference's sub-problem is -- admm_solver_v3.py:363-377
// takes any n; a second object keeps the builds parallel).
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>

#include "special_vertex.h"
#include "vertex_wg.h"
#include "vertex_wg_launch.h"

namespace {

using namespace gcsadmm_k;
using gcs_wg::WG_THREADS;

// (the diagnostic timing build gets the whole register file: with its stamps the n = 6 instantiation would spill at 256 registers,
//  and a spill next to the stamps' divergent branches is stored under a partial EXEC mask by this compiler -- measured: every
//  n = 6 solve failed in that build; the product build has no scratch, tests/test_build.py checks that)
#ifdef GCS_WG_TIMING
#define GCS_WG_MIN_BLOCKS 1
#else
#define GCS_WG_MIN_BLOCKS (gcs_wg::WG_THREADS <= 256 ? 2 : 1)
#endif
// diagnostic builds: -DGCS_WG_TIMING = region stamps (vertex_wg.h) + whole-solve ticks per workgroup; -DGCS_WG_BLOCKTIME = the
// whole-solve ticks alone (two s_memtime per solve: the low-overhead yardstick for A/B comparisons of the program)
#if defined(GCS_WG_TIMING) && !defined(GCS_WG_BLOCKTIME)
#define GCS_WG_BLOCKTIME 1
#endif
#ifdef GCS_WG_BLOCKTIME
__device__ unsigned long long g_wg_block_ticks[64], g_wg_block_iters[64];
#endif
// wavefronts per SIMD the register allocation must allow (HIP's second __launch_bounds__ argument is waves per execution unit; 512
// registers per SIMD lane): four at n = 2, 3 (<= 128 registers: with 256-thread workgroups four workgroups per CU, what
// gcsadmm_create's auto rule counts on; the allocator gets there without scratch once it is asked to), two at n = 6.  (The BOX
// instantiation at n = 6 needs three -- 47 KB of LDS fit three times -- and lands at 167 registers on its own; asking for three made
// the allocator spill 56 B, tests/test_build.py checks both.)
template <int N, bool BOX> constexpr int wg_min_blocks() { return GCS_WG_MIN_BLOCKS == 1 ? 1 : (N <= 3 ? 4 : 2); }
template <int N, class T, bool BOX>
__global__ __launch_bounds__(WG_THREADS, (wg_min_blocks<N, BOX>())) void vertex_wg_kernel(gcs_wg::WgArgs<T> a, SpecialArgs sp, const gcsadmm_control_block *cb)
{
    extern __shared__ __attribute__((aligned(16))) double smem[];
    if (cb->status != GCSADMM_RUNNING) return;
    const double rho = cb->rho, mu_scale = cb->mu_scale;
    if ((int)blockIdx.x >= a.n_vtx) {      // closed-form vertices, one per thread
        const int i = ((int)blockIdx.x - a.n_vtx) * WG_THREADS + (int)threadIdx.x;
        if (i < sp.count) {
            double *vals = smem + (sp.kind[i] == 2 ? 2 * MAX_SPECIAL_DEG : 0);   // source and target: own work arrays in LDS
            special_body<N, T>(a, sp, i, rho, mu_scale, vals, vals + MAX_SPECIAL_DEG);
        }
        return;
    }
    int status = 0, iters = 0;
#ifdef GCS_WG_BLOCKTIME
    const unsigned long long t_begin = __builtin_amdgcn_s_memtime();
#endif
    const int slot = a.order ? a.order[blockIdx.x] : (int)blockIdx.x;
    gcs_wg::wg_solve_vertex<N, T, BOX>(a, a.vtx[slot], rho, mu_scale, smem, status, iters);
    if (threadIdx.x == 0) {
        if (status != 0) atomicAdd(&a.counters[0], 1);
        atomicAdd(&a.counters[1], iters);
        if (a.unit_iters) a.unit_iters[slot] = iters;
#ifdef GCS_WG_BLOCKTIME
        if (blockIdx.x < 64) {      // whole-solve ticks and Newton iterations of the first 64 workgroups (which one ends the launch?)
            g_wg_block_ticks[blockIdx.x] += __builtin_amdgcn_s_memtime() - t_begin;
            g_wg_block_iters[blockIdx.x] += (unsigned long long)iters;
        }
#endif
    }
}

// SPLIT form of the same program (wg_solve_vertex<N, T, BOX, true>): workgroup b solves vtx[b] with its units in the device-memory slab
// units + unit_off[b] and only the fixed block and the polytope in LDS.  No closed-form vertices (they ride in the launch above), no
// slowest-first dispatch, no per-vertex iteration record: the launch holds the few vertices too large for the in-LDS form.  Built in the
// 256-thread objects only.  Its 64-bit unit addresses cost registers: at n = 8 the in-LDS bound (two waves per SIMD, 256 registers) spilled
// 36 bytes, so n = 7, 8 take one wave per SIMD (the vertices of this launch are few, and their LDS alone rarely leaves room for a second).
template <int N, bool BOX> constexpr int wg_split_min_blocks() { return N >= 7 ? 1 : wg_min_blocks<N, BOX>(); }
template <int N, class T, bool BOX>
__global__ __launch_bounds__(WG_THREADS, (wg_split_min_blocks<N, BOX>())) void vertex_wg_split_kernel(gcs_wg::WgArgs<T> a, WgSplitArgs w,
                                                                                              const gcsadmm_control_block *cb)
{
    extern __shared__ __attribute__((aligned(16))) double smem[];
    if (cb->status != GCSADMM_RUNNING) return;
    int status = 0, iters = 0;
    gcs_wg::wg_solve_vertex<N, T, BOX, true>(a, a.vtx[blockIdx.x], cb->rho, cb->mu_scale, smem, status, iters, w.units + w.unit_off[blockIdx.x]);
    if (threadIdx.x == 0) {
        if (status != 0) atomicAdd(&a.counters[0], 1);
        atomicAdd(&a.counters[1], iters);
    }
}

// The two kernel families of the program, by name.  Each has a BOX instantiation at n = 3 and 6: it pays from n = 3 (n = 6: -9 % per
// Newton iteration); at n = 2 the loops it shortens are two terms long and it measured 1 % slower, so n = 2 has none.
struct InLdsKernels { template <int N, class T, bool BOX> static constexpr auto kernel() { return vertex_wg_kernel<N, T, BOX>; } };
struct SplitKernels { template <int N, class T, bool BOX> static constexpr auto kernel() { return vertex_wg_split_kernel<N, T, BOX>; } };
template <int N> constexpr bool WG_HAS_BOX = N == 3 || N == 6;
// the state type of a launch (WgLaunchDesc::dtype)
template <class F> auto with_state(int dtype, F &&f) { return with_state_type(dtype == GCSADMM_F64, f); }

// one launch of family K: `extra` is the kernel's second argument (the closed-form vertices / the split form's workspace)
template <class K, int N, class T, class X>
void launch_kernels(const WgLaunchDesc &d, const gcs_wg::WgArgs<T> &a, unsigned grid, int lds, const X &extra, hipStream_t s)
{
    if constexpr (WG_HAS_BOX<N>) {
        if (d.box) { hipLaunchKernelGGL((K::template kernel<N, T, true>()), dim3(grid), dim3(WG_THREADS), lds, s, a, extra, d.step.cb); return; }
    }
    hipLaunchKernelGGL((K::template kernel<N, T, false>()), dim3(grid), dim3(WG_THREADS), lds, s, a, extra, d.step.cb);
}

// raise the dynamic-LDS limit of family K's instantiations (needed above 48 KB)
template <class K, int N> hipError_t set_lds(int dtype, int lds_bytes)
{
    return with_state(dtype, [&](auto t) {
        using T = decltype(t);
        hipError_t e = hipFuncSetAttribute((const void *)K::template kernel<N, T, false>(), hipFuncAttributeMaxDynamicSharedMemorySize, lds_bytes);
        if constexpr (WG_HAS_BOX<N>)
            if (e == hipSuccess) e = hipFuncSetAttribute((const void *)K::template kernel<N, T, true>(), hipFuncAttributeMaxDynamicSharedMemorySize, lds_bytes);
        return e;
    });
}

template <int N> void launch(const WgLaunchDesc &d, hipStream_t s)
{
    with_state(d.dtype, [&](auto t) {
        using T = decltype(t);
        gcs_wg::WgArgs<T> a;
        static_cast<StepArgs<T> &>(a) = d.step.typed<T>();
        a.n_vtx = d.n_vtx; a.vtx = d.vtx; a.order = d.order; a.unit_iters = d.unit_iters;
        const SpecialArgs sp{d.n_special, d.special_vtx, d.special_kind};
        const unsigned grid = (unsigned)(d.n_vtx + (d.n_special + WG_THREADS - 1) / WG_THREADS);
        if (grid == 0) return;
        const int lds = std::max(d.lds_bytes, (int)(4 * MAX_SPECIAL_DEG * sizeof(double)));
        launch_kernels<InLdsKernels, N, T>(d, a, grid, lds, sp, s);
    });
}

template <int N> void launch_split(const WgLaunchDesc &d, const WgSplitArgs &w, hipStream_t s)
{
    if (d.n_vtx <= 0) return;
    with_state(d.dtype, [&](auto t) {
        using T = decltype(t);
        gcs_wg::WgArgs<T> a;
        static_cast<StepArgs<T> &>(a) = d.step.typed<T>();
        a.n_vtx = d.n_vtx; a.vtx = d.vtx;
        launch_kernels<SplitKernels, N, T>(d, a, (unsigned)d.n_vtx, d.lds_bytes, w, s);
    });
}

// PROX configuration (admm_solver_v1.py:334-383): one workgroup per vertex, no edge blocks; the two trailing
// threads handle the terminals, which are points: x = (pt, pt), z = y (pt, pt), y = the minimiser of the remaining 1-D quadratic
// clamped to [0, 1] (the cone term vanishes: z_1 = z_2).
template <int N>
__global__ __launch_bounds__(WG_THREADS, 2) void vertex_prox_kernel(gcs_wg::WgArgs<double> a, int src, int dst)
{
    extern __shared__ __attribute__((aligned(16))) double smem[];
    constexpr int NX = 2 * N, NU = 4 * N + 1;
    if ((int)blockIdx.x >= a.n_vtx) {
        const int t = (int)threadIdx.x;
        const int v = t == 0 ? src : (t == 1 ? dst : -1);
        if (v < 0) return;
        const double *q = a.prox_q + (size_t)v * NU, *c = a.prox_c + (size_t)v * NU;
        double num = q[2 * NX] * c[2 * NX], den = q[2 * NX];
        for (int k = 0; k < NX; ++k) {
            const double pt = a.center[(size_t)v * N + (k < N ? k : k - N)];
            num += q[NX + k] * pt * c[NX + k];
            den += q[NX + k] * pt * pt;
        }
        double y = den > 0.0 ? num / den : 0.5;
        y = y < 0.0 ? 0.0 : (y > 1.0 ? 1.0 : y);
        for (int k = 0; k < NX; ++k) {
            const double pt = a.center[(size_t)v * N + (k < N ? k : k - N)];
            a.xv[(size_t)v * NX + k] = pt;
            a.zv[(size_t)v * NX + k] = y * pt;
        }
        a.yv[v] = y;
        return;
    }
    int status = 0, iters = 0;
    gcs_wg::wg_solve_vertex<N, double>(a, a.vtx[blockIdx.x], 1.0, 1.0, smem, status, iters);
    if (threadIdx.x == 0 && a.counters) {
        if (status != 0) atomicAdd(&a.counters[0], 1);
        atomicAdd(&a.counters[1], iters);
    }
}

template <int N> void launch_prox(const WgLaunchDesc &d, const double *q, const double *c, int src, int dst, hipStream_t s)
{
    gcs_wg::WgArgs<double> a{};
    static_cast<StepArgs<double> &>(a) = d.step.typed<double>();
    a.n_vtx = d.n_vtx; a.vtx = d.vtx; a.prox_q = q; a.prox_c = c;
    if (d.lds_bytes > 48 * 1024)
        (void)hipFuncSetAttribute((const void *)vertex_prox_kernel<N>, hipFuncAttributeMaxDynamicSharedMemorySize, d.lds_bytes);
    hipLaunchKernelGGL((vertex_prox_kernel<N>), dim3(d.n_vtx + 1), dim3(WG_THREADS), d.lds_bytes, s, a, src, dst);
}

}  // namespace
