// terminal_region.hip -- x-update of terminals that are regions (terminal_region.h): one workgroup of 64 or 256 threads per terminal, launched on
// the handle's auxiliary stream beside the vertex-step launch (gcsadmm.hip launch_vertex), or, for the members of a batch, one launch per
// group of terminals on the batch's (launch_batch_iteration).  Own object: the vertex kernels are not touched.
#include <hip/hip_runtime.h>

#include "gcsadmm.h"
#include "terminal_launch.h"
#include "terminal_region.h"

namespace gcsadmm_k {

constexpr int TERM_THREADS = 256;

// executor of terminal_region_solve on the device: one workgroup of 64 or 256 threads; reductions by wavefront shuffles in a fixed order
// (bit-reproducible), across wavefronts through LDS
#ifdef GCS_TERM_TIMING
__device__ unsigned long long g_term_cycles[32], g_term_visits[32];      // diagnostic build: ticks per phase of the solve, workgroup 0
#endif
struct TermExec {
    double *red;      // [3 * 4]
#ifdef GCS_TERM_TIMING
    unsigned long long last = 0;
    __device__ __forceinline__ void stamp(int k)
    {
        __builtin_amdgcn_sched_barrier(0);
        const unsigned long long t = __builtin_amdgcn_s_memtime();
        if (threadIdx.x == 0 && blockIdx.x == 0 && last) { atomicAdd(&g_term_cycles[k], t - last); atomicAdd(&g_term_visits[k], 1ull); }
        last = __builtin_amdgcn_s_memtime();
    }
#else
    __device__ __forceinline__ void stamp(int) {}
#endif
    __device__ __forceinline__ int tid() const { return (int)threadIdx.x; }
    __device__ __forceinline__ int nthreads() const { return (int)blockDim.x; }
    __device__ __forceinline__ void sync() { __syncthreads(); }
    __device__ __forceinline__ void reduce3(double &mn, double &s1, double &s2)
    {
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) {
            mn = fmin(mn, __shfl_xor(mn, off, 64));
            s1 += __shfl_xor(s1, off, 64);
            s2 += __shfl_xor(s2, off, 64);
        }
        const int nw = (int)blockDim.x >> 6;
        if (nw > 1) {
            const int w = (int)threadIdx.x >> 6;
            if ((threadIdx.x & 63) == 0) { red[w] = mn; red[4 + w] = s1; red[8 + w] = s2; }
            __syncthreads();
            mn = red[0]; s1 = red[4]; s2 = red[8];
            for (int k = 1; k < nw; ++k) { mn = fmin(mn, red[k]); s1 += red[4 + k]; s2 += red[8 + k]; }
            __syncthreads();
        }
    }
};

// The solve of terminal `ti` of the handle that (a, t, cb) describe, by the calling workgroup: the body of both kernels below, so that a
// terminal solved in a batch launch is the same instructions on the same arguments as in its handle's own launch.  A handle that has
// stopped leaves before any barrier or LDS use.  TB is TermBlock as the kernel holds it: a kernel argument, or a table entry in the
// constant address space -- `ti` indexes its arrays, and an index the compiler cannot resolve into a private copy would cost scratch.
// The LDS objects are the calling kernel's own, so that each kernel lays out its LDS as if the other did not exist.
// LDSWS: the work arrays live in dynamic LDS (its own instantiation, so that the compiler addresses them as LDS rather than through flat pointers)
template <int N, class T, bool LDSWS, class TB>
__device__ __forceinline__ void terminal_region_body(const StepArgs<T> &a, TB &t, const gcsadmm_control_block *cb, const int ti,
                                                     gcs_term::TermShared<N> &sh, double *red, double *term_lds)
{
    if (cb->status != GCSADMM_RUNNING) return;
    const int v = t.vtx[ti];
    gcs_term::TermProblem<T> P;
    const int p0 = a.poly_ptr[v], lo = a.inc_ptr[v];
    P.m = a.poly_ptr[v + 1] - p0; P.d = a.inc_ptr[v + 1] - lo; P.d_in = a.deg_in[v]; P.is_src = t.is_src[ti];
    P.A = a.poly_A + (size_t)p0 * N; P.bc = a.poly_bc + p0; P.cen = a.center + (size_t)v * N;
    P.inc_edge = a.inc_edge + lo; P.inc_lo = lo;
    P.E = a.E; P.NI = a.NI; P.edge_major = a.edge_major;
    P.zedge = a.zedge; P.mu = a.mu; P.copy = a.copy;
    P.xv = a.xv + (size_t)v * 2 * N; P.zv = a.zv + (size_t)v * 2 * N; P.yv = a.yv + v;
    P.rho = cb->rho; P.mu_scale = cb->mu_scale; P.eps_edge = a.eps_edge; P.ipm_tol = a.ipm_tol; P.ipm_max_iter = a.ipm_max_iter;
    P.warm = t.rec ? t.rec + t.rec_off[ti] : nullptr;
    TermExec ex{red};
    // work arrays: LDS when the launch was given room for the larger of the terminals (lds_doubles), the HBM workspace otherwise
    int r;
    if constexpr (LDSWS) r = gcs_term::terminal_region_solve<N, T>(ex, P, term_lds, sh);
    else r = gcs_term::terminal_region_solve<N, T>(ex, P, t.ws + t.ws_off[ti], sh);
    if (threadIdx.x == 0) {
        if (r < 0) atomicAdd(&a.counters[0], 1);
        else atomicAdd(&a.counters[1], r);
    }
}

// one handle: workgroup blockIdx.x solves its terminal blockIdx.x
template <int N, class T, bool LDSWS>
__global__ __launch_bounds__(TERM_THREADS) void terminal_region_kernel(StepArgs<T> a, TermBlock t, const gcsadmm_control_block *cb)
{
    extern __shared__ __attribute__((aligned(16))) double term_lds[];
    __shared__ gcs_term::TermShared<N> sh;
    __shared__ double red[12];
    terminal_region_body<N, T, LDSWS, const TermBlock>(a, t, cb, (int)blockIdx.x, sh, red, term_lds);
}

// BATCH form (gcsadmm_batch_run on a batch made with GCSADMM_BATCH_TERMINALS): workgroup blockIdx.x solves entry blockIdx.x of the
// table, one entry per TERMINAL of the launch's group -- the kernarg of the solo launch of that terminal's handle and the terminal's
// index in it.  The table is written by the host before the launch and by nobody during it: it is read through the constant address
// space, as kernel arguments are (vertex_wave_batch_kernel.h).  The index is uniform over the workgroup, so the entry comes in through
// scalar loads.  The launch's thread count and LDSWS are those of every member of the group (batch_plan.h groups by them).
template <int N, class T, bool LDSWS>
__global__ __launch_bounds__(TERM_THREADS) void terminal_region_batch_kernel(const TermBatchEntry<T> *__restrict__ table)
{
    extern __shared__ __attribute__((aligned(16))) double term_lds[];
    __shared__ gcs_term::TermShared<N> sh;
    __shared__ double red[12];
    using Entry = const __attribute__((address_space(4))) TermBatchEntry<T>;
    __builtin_assume_dereferenceable(table + blockIdx.x, sizeof(Entry));
    Entry &e = *((Entry *)table + blockIdx.x);
    const StepArgs<T> a = *(const StepArgs<T> *)&e.a;
    terminal_region_body<N, T, LDSWS, const __attribute__((address_space(4))) TermBlock>(a, e.t, e.cb, e.ti, sh, red, term_lds);
}

template <int N, class T> static void launch_n(const TermLaunchDesc &d, hipStream_t s)
{
    const size_t lds = (size_t)d.lds_doubles * sizeof(double);
    if (lds) hipLaunchKernelGGL((terminal_region_kernel<N, T, true>), dim3(d.count), dim3(d.threads), lds, s, d.step.typed<T>(), d.t, d.step.cb);
    else hipLaunchKernelGGL((terminal_region_kernel<N, T, false>), dim3(d.count), dim3(d.threads), 0, s, d.step.typed<T>(), d.t, d.step.cb);
}

template <int N, class T> static void launch_batch_n(const TermBatchLaunch &b, hipStream_t s)
{
    const size_t lds = (size_t)b.lds_doubles * sizeof(double);
    const auto *table = (const TermBatchEntry<T> *)b.table;
    if (lds) hipLaunchKernelGGL((terminal_region_batch_kernel<N, T, true>), dim3(b.count), dim3(b.threads), lds, s, table);
    else hipLaunchKernelGGL((terminal_region_batch_kernel<N, T, false>), dim3(b.count), dim3(b.threads), 0, s, table);
}

}  // namespace gcsadmm_k

#ifdef GCS_TERM_TIMING
extern "C" int gcsadmm_debug_term_cycles(unsigned long long *cycles32, unsigned long long *visits32)
{
    int e = (int)hipMemcpyFromSymbol(cycles32, HIP_SYMBOL(gcsadmm_k::g_term_cycles), 32 * sizeof(unsigned long long));
    if (e == 0) e = (int)hipMemcpyFromSymbol(visits32, HIP_SYMBOL(gcsadmm_k::g_term_visits), 32 * sizeof(unsigned long long));
    return e;
}
#endif

long long gcsadmm_terminal_ws_doubles(int n, int facets, int live_edges) { return gcs_term::terminal_ws_doubles(n, facets, live_edges); }
long long gcsadmm_terminal_record_doubles(int n, int facets, int live_edges) { return gcs_term::terminal_record_doubles(n, facets, live_edges); }

void gcsadmm_terminal_launch(const gcsadmm_k::TermLaunchDesc &d, hipStream_t s)
{
    using namespace gcsadmm_k;
    if (d.count <= 0) return;
    dispatch_dim<1, 2, 3, 4, 5, 6, 7, 8>(d.n, [&](auto n) {
        constexpr int N = decltype(n)::value;
        if (d.dtype == GCSADMM_F64) launch_n<N, double>(d, s);
        else launch_n<N, float>(d, s);
    });
}

size_t gcsadmm_terminal_batch_entry_bytes(int dtype)
{
    return dtype == GCSADMM_F64 ? sizeof(gcsadmm_k::TermBatchEntry<double>) : sizeof(gcsadmm_k::TermBatchEntry<float>);
}

void gcsadmm_terminal_batch_fill(const gcsadmm_k::TermLaunchDesc &d, int ti, void *entry_host)
{
    using namespace gcsadmm_k;
    if (d.dtype == GCSADMM_F64) *(TermBatchEntry<double> *)entry_host = TermBatchEntry<double>{d.step.typed<double>(), d.t, d.step.cb, ti};
    else *(TermBatchEntry<float> *)entry_host = TermBatchEntry<float>{d.step.typed<float>(), d.t, d.step.cb, ti};
}

void gcsadmm_terminal_launch_batch(const gcsadmm_k::TermBatchLaunch &b, hipStream_t s)
{
    using namespace gcsadmm_k;
    if (b.count <= 0) return;
    dispatch_dim<1, 2, 3, 4, 5, 6, 7, 8>(b.n, [&](auto n) {
        constexpr int N = decltype(n)::value;
        if (b.dtype == GCSADMM_F64) launch_batch_n<N, double>(b, s);
        else launch_batch_n<N, float>(b, s);
    });
}
