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
// what one workgroup of a vertex-step launch does once it knows its arguments: workgroup bx of the launch solves its generic vertex, the
// trailing workgroups take the closed-form vertices.  One body for the kernel that gets its arguments in the kernarg segment
// (vertex_wg_kernel) and the one that reads them from a table (vertex_wg_batch_kernel): the same instructions on the same numbers.
template <int N, class T, bool BOX>
__device__ __forceinline__ void vertex_wg_body(const gcs_wg::WgArgs<T> &a, const SpecialArgs &sp, double rho, double mu_scale, int bx, double *smem)
{
    if (bx >= a.n_vtx) {      // closed-form vertices, one per thread
        const int i = (bx - a.n_vtx) * WG_THREADS + (int)threadIdx.x;
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
    const int slot = a.order ? a.order[bx] : bx;
    gcs_wg::wg_solve_vertex<N, T, BOX>(a, a.vtx[slot], rho, mu_scale, smem, status, iters);
    if (threadIdx.x == 0) {
        if (status != 0) atomicAdd(&a.counters[0], 1);
        atomicAdd(&a.counters[1], iters);
        if (a.unit_iters) a.unit_iters[slot] = iters;
#ifdef GCS_WG_BLOCKTIME
        if (bx < 64) {      // whole-solve ticks and Newton iterations of the first 64 workgroups (which one ends the launch?)
            g_wg_block_ticks[bx] += __builtin_amdgcn_s_memtime() - t_begin;
            g_wg_block_iters[bx] += (unsigned long long)iters;
        }
#endif
    }
}

// FUSED TAIL (graphs whose edges fit one edge workgroup, CreatePlan::fused_tail): the iteration is ONE launch.  Every workgroup of the
// launch, once its vertices are solved, PUBLISHES -- its copy columns were stored write-through (sc1: store_copy, step_args.h), every
// wavefront drains its stores (s_waitcnt vmcnt(0)), one workgroup barrier -- and ARRIVES: thread 0, whose counter adds are drained too,
// makes one relaxed agent-scope add on the handle's ticket.  (The trailing workgroups of the closed-form vertices keep their plain
// stores -- as sc1 stores inside special_body's divergent loops they cost every instantiation 3-4 vector registers of spilled scalars
// across the Newton loop, and the n = 6 BOX instantiation its third wavefront per SIMD -- and thread 0 writes them back with one
// agent-scope release before its add.  Those workgroups are done within a few microseconds of a launch that lasts as long as its
// slowest interior-point solve, so the release is never on the critical path.)  The workgroup whose add returns gridDim.x - 1 came last: every other
// workgroup has published, so it runs edge_kernel's MODE 1 body (edge_step.h) on threads 0 .. EDGE_BLOCK - 1 with sc1 loads of the
// copies, then the control step, and leaves the ticket at 0.  Nobody waits for anybody: no spin, no flag poll, no cooperative launch,
// and no fence in a workgroup that solves -- the hand-off is MI355X_MICROARCH.md's "sc1 stores, drain, counter add; the last adder reads with sc1 loads", the
// one edge_kernel MODE 2 uses for its partials (a release fence would write back the XCD's L2: 3.5 us, more than the launch saved).
// zedge and mu were written by the previous launch and are read by plain loads; the tail's own stores to them are read by the next.
template <class T> struct WgTail {
    int enabled;
    EdgeArgs<T> edge;
    gcsadmm_control_block *cb;
    double *sums;
    ControlParams cp;
    int *counters;
    double *trace;
    unsigned *ticket;
};

template <class T, int C>
__device__ __forceinline__ void wg_fused_tail(const WgTail<T> &t, double mu_scale, bool closed_form, double *smem)
{
    // the edge's two state columns do not depend on the solves: loaded while the stores drain
    const EdgePre pre = edge_prefetch(t.edge, mu_scale);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");      // this wavefront's copy stores (and thread 0's counter adds) have left
    __syncthreads();                                         // every wavefront's have; and the LDS of the solve is free
    double(*red)[5] = (double(*)[5])smem;
    int *is_last = (int *)(smem + EDGE_BLOCK / EDGE_WAVE * 5);
    if (threadIdx.x == 0) {
        if (closed_form) {      // plain stores: written back by one release, drained
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        }
        const unsigned k = __hip_atomic_fetch_add(t.ticket, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        *is_last = (k == gridDim.x - 1);
    }
    __syncthreads();
    if (!*is_last) return;
    edge_body<T, 1, C, 1, EdgeInTail>(t.edge, t.cb, t.sums, t.cp, t.counters, t.trace, t.ticket, 0, 1, red, is_last, pre);
    if (threadIdx.x == 0) __hip_atomic_store(t.ticket, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);     // ready for the next launch
}

// REGISTERS: the kernel reads its tail block LATE.  The Newton loop's scalar registers already spill into vector lanes, and nothing of the
// tail may be live in it.  So after the solve the kernel takes the address of its own kernarg segment, makes it opaque, and reads the
// block (twenty words) -- and through it the dual scale for the tail -- from there through the constant address space: scalar loads
// where they are needed (vertex_wg_batch_kernel reads its table the same way, for the same reason).  Every instantiation keeps the
// register count it had without the tail, except n = 2 f64 (97 -> 115, the tail's own loads: same occupancy class).
template <class T> constexpr size_t wg_tail_kernarg_offset()
{
    static_assert(alignof(gcs_wg::WgArgs<T>) == 8 && alignof(SpecialArgs) == 8 && alignof(WgTail<T>) == 8, "kernarg layout: every argument starts on 8 bytes");
    return sizeof(gcs_wg::WgArgs<T>) + sizeof(SpecialArgs) + sizeof(const gcsadmm_control_block *);
}

template <int N, class T, bool BOX>
__global__ __launch_bounds__(WG_THREADS, (wg_min_blocks<N, BOX>())) void vertex_wg_kernel(gcs_wg::WgArgs<T> a, SpecialArgs sp, const gcsadmm_control_block *cb,
                                                                                 WgTail<T> /* read late, below */)
{
    extern __shared__ __attribute__((aligned(16))) double smem[];
    if (cb->status != GCSADMM_RUNNING) return;
    vertex_wg_body<N, T, BOX>(a, sp, cb->rho, cb->mu_scale, (int)blockIdx.x, smem);
    typedef const __attribute__((address_space(4))) char *KernargPtr;
    KernargPtr kp = (KernargPtr)__builtin_amdgcn_kernarg_segment_ptr();
    asm volatile("" : "+s"(kp));
    typedef const __attribute__((address_space(4))) WgTail<T> *TailPtr;
    TailPtr tp = (TailPtr)(kp + wg_tail_kernarg_offset<T>());
    if (!tp->enabled) return;      // (uniform over the launch: a kernel argument)
    const WgTail<T> tail = *(const WgTail<T> *)tp;
    // the dual scale the launch started with: the control block is not written before the tail's own control step
    const double mu_scale = __hip_atomic_load(&tail.cb->mu_scale, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    wg_fused_tail<T, 2 * N + 1>(tail, mu_scale, (int)blockIdx.x >= a.n_vtx, smem);
}

#if GCS_WG_THREADS == 256
// BATCH form (gcsadmm_batch_run): one launch serves many handles.  Row blockIdx.y of the grid is member blockIdx.y of the batch: the
// workgroup copies that member's entry of the table -- the arguments vertex_wg_kernel gets in its kernarg segment, the member's own
// control block and the width of its own grid -- and runs the body above on it.  The index is uniform over the workgroup, so the entry
// comes in through scalar loads and lives in scalar registers as kernel arguments do.  Workgroups beyond the member's own grid (the
// launch is as wide as the widest member) and those of a member that has stopped leave at once: the whole workgroup, before any barrier
// or LDS use.  Built in the 256-thread objects only.
template <class T> struct WgBatchEntry {
    gcs_wg::WgArgs<T> a;
    SpecialArgs sp;
    const gcsadmm_control_block *cb;
    int grid_x;                 // workgroups of this member: n_vtx + ceil(n_special / 256)
};
template <int N, class T, bool BOX>
__global__ __launch_bounds__(WG_THREADS, (wg_min_blocks<N, BOX>())) void vertex_wg_batch_kernel(const WgBatchEntry<T> *__restrict__ table)
{
    extern __shared__ __attribute__((aligned(16))) double smem[];
    // the table is written by the host before the launch and by nobody during it: it is read through the constant address space, as
    // kernel arguments are, so that the compiler may reload a field where it needs it instead of keeping all of them live (read as
    // plain global memory the entry cost 90 more registers and 250 bytes of scratch per lane)
    __builtin_assume_dereferenceable(table + blockIdx.y, sizeof(WgBatchEntry<T>));
    const WgBatchEntry<T> e = *(const WgBatchEntry<T> *)((const __attribute__((address_space(4))) WgBatchEntry<T> *)table + blockIdx.y);
    if ((int)blockIdx.x >= e.grid_x || e.cb->status != GCSADMM_RUNNING) return;
    vertex_wg_body<N, T, BOX>(e.a, e.sp, e.cb->rho, e.cb->mu_scale, (int)blockIdx.x, smem);
}
#endif

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
#if GCS_WG_THREADS == 256
struct BatchKernels { template <int N, class T, bool BOX> static constexpr auto kernel() { return vertex_wg_batch_kernel<N, T, BOX>; } };
#endif
template <int N> constexpr bool WG_HAS_BOX = N == 3 || N == 6;
// the state type of a launch (WgLaunchDesc::dtype)
template <class F> auto with_state(int dtype, F &&f) { return with_state_type(dtype == GCSADMM_F64, f); }

// one launch of family K: `extra` is the kernel's second argument (the closed-form vertices / the split form's workspace)
// (`more`: the kernel's arguments after the control block -- the in-LDS family's tail)
template <class K, int N, class T, class X, class... More>
void launch_kernels(const WgLaunchDesc &d, const gcs_wg::WgArgs<T> &a, unsigned grid, int lds, const X &extra, hipStream_t s, const More &...more)
{
    if constexpr (WG_HAS_BOX<N>) {
        if (d.box) { hipLaunchKernelGGL((K::template kernel<N, T, true>()), dim3(grid), dim3(WG_THREADS), lds, s, a, extra, d.step.cb, more...); return; }
    }
    hipLaunchKernelGGL((K::template kernel<N, T, false>()), dim3(grid), dim3(WG_THREADS), lds, s, a, extra, d.step.cb, more...);
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

// the typed arguments of an in-LDS launch (the kernarg of vertex_wg_kernel, or a member's entry of the batch table)
template <class T> gcs_wg::WgArgs<T> in_lds_args(const WgLaunchDesc &d)
{
    gcs_wg::WgArgs<T> a;
    static_cast<StepArgs<T> &>(a) = d.step.typed<T>();
    a.n_vtx = d.n_vtx; a.vtx = d.vtx; a.order = d.order; a.unit_iters = d.unit_iters;
    return a;
}

// the typed tail of an in-LDS launch (its last kernel argument)
template <class T> WgTail<T> in_lds_tail(const WgTailDesc &d)
{
    return WgTail<T>{d.enabled, retype<T>(d.edge), d.cb, d.sums, d.cp, d.counters, d.trace, d.ticket};
}

template <int N> void launch(const WgLaunchDesc &d, hipStream_t s)
{
    with_state(d.dtype, [&](auto t) {
        using T = decltype(t);
        gcs_wg::WgArgs<T> a = in_lds_args<T>(d);
        a.publish = d.tail.enabled;      // the copies go out write-through exactly when the launch has a reader for them
        const SpecialArgs sp{d.n_special, d.special_vtx, d.special_kind};
        const unsigned grid = (unsigned)(d.n_vtx + (d.n_special + WG_THREADS - 1) / WG_THREADS);
        if (grid == 0) return;
        launch_kernels<InLdsKernels, N, T>(d, a, grid, wg_launch_lds_bytes(d.lds_bytes, d.tail.enabled != 0), sp, s, in_lds_tail<T>(d.tail));
    });
}

#if GCS_WG_THREADS == 256
// one launch for the whole batch: grid (widest member, members), the LDS of the largest member
template <int N> void launch_batch(const WgBatchLaunch &b, hipStream_t s)
{
    with_state(b.dtype, [&](auto t) {
        using T = decltype(t);
        const auto *table = (const WgBatchEntry<T> *)b.table;
        if constexpr (WG_HAS_BOX<N>) {
            if (b.box) { hipLaunchKernelGGL((vertex_wg_batch_kernel<N, T, true>), dim3(b.grid_x, b.count), dim3(WG_THREADS), b.lds_bytes, s, table); return; }
        }
        hipLaunchKernelGGL((vertex_wg_batch_kernel<N, T, false>), dim3(b.grid_x, b.count), dim3(WG_THREADS), b.lds_bytes, s, table);
    });
}
#endif

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
