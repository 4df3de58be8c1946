// edge_step.h -- the edge step (z-update, dual update, five partial norms: admm_solver_v3.py:543-614) and the control step
// (admm_solver_v3.py:697-733) as device functions, shared by the objects that run them: gcsadmm.hip (edge_kernel, edge_batch_kernel,
// control_kernel: loop_kernels.h) and the workgroup program's objects, where on small graphs the last vertex workgroup to finish runs the single-workgroup
// edge step as the tail of the vertex launch (vertex_wg_kernel.h, FUSED TAIL).  One body, so that every caller runs the same
// instructions on the same numbers in the same order.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "gcsadmm.h"
#include "step_args.h"

namespace gcsadmm_k {

constexpr int EDGE_WAVE = 64;            // lanes per wavefront (gfx950)

// -------------------------------------------------------------------------------------------------
// edge step: one thread per directed edge, all c coupled words
// -------------------------------------------------------------------------------------------------
template <class T> struct EdgeArgs {
    int E, NI, c;
    const int *edge_inc_tail, *edge_inc_head;
    const uint8_t *inc_counted, *edge_counted;   // may be null
    const T *copy;
    T *zedge, *mu;
    double *partials;    // [gridDim.x][5]
};
// the same arguments with the state pointers as another type (host side: the handle's dtype picks T at launch, as StepDesc::typed)
template <class U, class V> EdgeArgs<U> retype(const EdgeArgs<V> &a)
{
    return EdgeArgs<U>{a.E, a.NI, a.c, a.edge_inc_tail, a.edge_inc_head, a.inc_counted, a.edge_counted, (const U *)a.copy, (U *)a.zedge, (U *)a.mu, a.partials};
}

__device__ __forceinline__ double wave_sum(double v)
{
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
    return v;
}

// dual update mu_scale * mu + r with the product rounded ON ITS OWN: left to the compiler the line contracts into an fma, and for a
// mu_scale that is not a power of two (tau_incr = 3) the result then differs from the two-rounding value in a few percent of the words --
// by up to one ulp of mu_new, which the per-word bound of tests/loop_reference.py does not always have room for.  With a power of two
// (every default run) the product is exact and both forms give the same bits.
__device__ __forceinline__ double scaled_plus(double scale, double x, double r)
{
#pragma clang fp contract(off)
    return scale * x + r;
}

struct ControlParams {
    double tau_incr, tau_decr, nu, eps_abs, eps_rel, nx, nmu;
    int it_rho_limit, max_it;
};

// WHERE the body runs.  InKernel: a launch of its own (edge_kernel, edge_batch_kernel: EDGE_BLOCK threads, every thread may take an
// edge; the vertex step's copies and counters came through a kernel boundary, so plain loads see them).  InTail: the tail of the
// vertex-step launch that wrote the copies -- they were published with write-through (sc1) stores and are read with agent-scope
// relaxed (sc1) loads, as are the counters the other workgroups added to; the workgroup may be wider than EDGE_BLOCK (512 threads):
// the threads beyond take no edge and add nothing, but reach every barrier.  Both barriers are __syncthreads().
struct EdgeInKernel {
    static constexpr bool TAIL = false;
    template <class T> static __device__ __forceinline__ T load_copy(const T *p) { return *p; }
    static __device__ __forceinline__ int load_counter(const int *p) { return *p; }
    static __device__ __forceinline__ void store_counter(int *p, int v) { *p = v; }
    static __device__ __forceinline__ bool edge_thread() { return true; }
    static __device__ __forceinline__ void sync() { __syncthreads(); }
};
struct EdgeInTail {
    static constexpr bool TAIL = true;
    template <class T> static __device__ __forceinline__ T load_copy(const T *p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
    static __device__ __forceinline__ int load_counter(const int *p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
    static __device__ __forceinline__ void store_counter(int *p, int v) { __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
    static __device__ __forceinline__ bool edge_thread() { return threadIdx.x < (unsigned)EDGE_BLOCK; }
    static __device__ __forceinline__ void sync() { __syncthreads(); }
};

// what the tail loads BEFORE it waits for the other workgroups (nothing of it depends on the solves): the two state columns of the
// thread's edge, and the dual scale the launch started with (the control block is not written before the tail's own control step)
struct EdgePre {
    int it = 0, ih = 0;
    double mu_scale = 1.0;
};
template <class T> __device__ __forceinline__ EdgePre edge_prefetch(const EdgeArgs<T> &a, double mu_scale)
{
    EdgePre p;
    p.mu_scale = mu_scale;
    if (threadIdx.x < (unsigned)EDGE_BLOCK && a.E > 0) {
        const int e = (int)threadIdx.x, ee = e < a.E ? e : a.E - 1;
        p.it = a.edge_inc_tail ? a.edge_inc_tail[ee] : ee; p.ih = a.edge_inc_head ? a.edge_inc_head[ee] : a.E + ee;
    }
    return p;
}

// admm_solver_v3.py:697-733 on the five (globally reduced) sums; one thread
// global_fails: the inner-failure count comes with the (all-reduced) sums as sums[5] instead of from this handle's counter
template <class P = EdgeInKernel>
__device__ void control_body(gcsadmm_control_block *cb, const double *sums, const ControlParams &p, int *counters, double *trace,
                             bool global_fails = false)
{
    if (cb->status != GCSADMM_RUNNING) return;
    double s[5];
    for (int k = 0; k < 5; ++k) { s[k] = sums[k]; cb->sums[k] = s[k]; }
    const int it = cb->it;
    double rho = cb->rho;
    const int fails = global_fails ? (int)(sums[5] + 0.5) : P::load_counter(&counters[0]), iters = P::load_counter(&counters[1]);
    P::store_counter(&counters[0], 0); P::store_counter(&counters[1], 0);
    cb->inner_failures = fails; cb->inner_iters = iters;
    const double tot = s[0] + s[1] + s[2] + s[3] + s[4];
    if (!(fabs(tot) <= 1.7976931348623157e308)) {   // non-finite iterate (NaN or an overflowed total): admm_solver_v3.py:662-664, 679-681
        cb->status = GCSADMM_DIVERGED;
        return;
    }
    const double pri = sqrt(s[0]), dual = rho * sqrt(2.0 * s[1]);
    double mu_scale = 1.0;
    if (pri >= p.nu * dual && it < p.it_rho_limit) { rho *= p.tau_incr; mu_scale = 1.0 / p.tau_incr; }
    else if (dual >= p.nu * pri && it < p.it_rho_limit) { rho *= 1.0 / p.tau_decr; mu_scale = p.tau_incr; }
    const double eps_pri = sqrt(p.nx) * p.eps_abs + p.eps_rel * fmax(sqrt(s[2]), sqrt(2.0 * s[3]));
    const double eps_dual = sqrt(p.nmu) * p.eps_abs + p.eps_rel * mu_scale * sqrt(s[4]);
    cb->rho = rho; cb->mu_scale = mu_scale;
    cb->pri = pri; cb->dual = dual; cb->eps_pri = eps_pri; cb->eps_dual = eps_dual;
    if (trace) {
        double *tr = trace + (size_t)(it - 1) * 6;
        tr[0] = rho; tr[1] = pri; tr[2] = dual; tr[3] = eps_pri; tr[4] = eps_dual; tr[5] = (double)fails;
    }
    if (pri < eps_pri && dual < eps_dual) { cb->status = GCSADMM_CONVERGED; return; }
    cb->it = it + 1;
    if (it + 1 > p.max_it) cb->status = GCSADMM_MAX_IT;
}

// edges a thread of the edge kernel has in flight at once on LARGE graphs (registers: U x 5C words); which graphs use it:
// edge_unroll_rt (create_plan.h)
template <class T, int C> __host__ __device__ constexpr int edge_unroll() { return sizeof(T) == 4 ? (C <= 7 ? 4 : 2) : (C <= 7 ? 2 : 1); }

// word w of edge e (state columns it, ih), from the five loaded values: the new edge copy, the two duals, the contributions to the sums
template <class T>
__device__ __forceinline__ void edge_word(const EdgeArgs<T> &a, int w, int e, int it, int ih, T cu_t, T cw_t, T zo_t, T mu_t, T mw_t, double mu_scale,
                                          double we, double wt, double wh, double (&s)[5])
{
    const double cu = (double)cu_t, cw = (double)cw_t, zo = (double)zo_t;
    const T zn_t = (T)(0.5 * (cu + cw));
    const double zn = (double)zn_t;
    const double ru = cu - zn, rw = cw - zn;
    const T mu_u_t = (T)scaled_plus(mu_scale, (double)mu_t, ru);
    const T mu_w_t = (T)scaled_plus(mu_scale, (double)mw_t, rw);
    a.mu[(size_t)w * a.NI + it] = mu_u_t;
    a.mu[(size_t)w * a.NI + ih] = mu_w_t;
    a.zedge[(size_t)w * a.E + e] = zn_t;
    const double mu_u = (double)mu_u_t, mu_w = (double)mu_w_t;
    s[0] += wt * ru * ru + wh * rw * rw;
    s[1] += we * (zn - zo) * (zn - zo);
    s[2] += wt * cu * cu + wh * cw * cw;
    s[3] += we * zn * zn;
    s[4] += wt * mu_u * mu_u + wh * mu_w * mu_w;
}

// words of an edge the TAIL form has in flight at once: all 5 x C loads of edge_kernel would set the register count of the vertex kernel
// whose tail it is (n = 6, f64: 210 against the solve's 167), so the tail takes the words in groups
#ifndef GCS_TAIL_WORDS
#define GCS_TAIL_WORDS 5
#endif
template <class T, int C> __host__ __device__ constexpr int tail_words() { return C < GCS_TAIL_WORDS ? C : GCS_TAIL_WORDS; }

// MODE 0: partial sums per workgroup only (gcsadmm_edge_step: the caller all-reduces / finalizes);
// MODE 1: single workgroup (at most EDGE_BLOCK edges, gcsadmm_run on small graphs): the workgroup also does the final
//         reduction and the control step;
// MODE 2: any grid (gcsadmm_run): the LAST workgroup to finish -- told by an agent-scope ticket counter -- reduces all the
//         partials in the fixed order of finalize_kernel and runs the control step: one launch per edge step instead of two;
// MODE 3: as MODE 2 without the control step (gcsadmm_run_partitioned): the last workgroup leaves the five sums and, in
//         sums[5], this partition's inner-failure count for the all-reduce that follows.
// C = coupled words per copy (2n+1), compile-time so that all C x 5 loads of an edge are in flight at once.
// The body is a function of the arguments, the workgroup's index bx and the number of workgroups nblocks that share the edges, so that
// the kernel that gets them from its kernarg segment and its grid (edge_kernel) and the one that reads them from a table
// (edge_batch_kernel) run the same instructions on the same numbers.  red / is_last: the workgroup's LDS, declared by the caller
// (MODE 1 uses red[0 .. EDGE_BLOCK / 64) only).
// P = EdgeInTail (MODE 1, U = 1, bx = 0, nblocks = 1): the body as the tail of the vertex-step launch, with `pre` loaded beforehand;
// the thread-to-edge map, the wavefront sums, red[wv][k] and the serial sum over the four wavefronts are MODE 1's, so the five sums
// come out bit for bit; the control step takes them from red[0] (LDS) instead of reading sums[] back.
template <class T, int MODE, int C, int U, class P = EdgeInKernel>
__device__ __forceinline__ void edge_body(const EdgeArgs<T> &a, gcsadmm_control_block *cb, double *sums, const ControlParams &cp, int *counters,
                                          double *trace, unsigned *ticket, const unsigned bx, const unsigned nblocks, double (*red)[5], int *is_last,
                                          const EdgePre &pre = EdgePre())
{
    static_assert(!P::TAIL || (MODE == 1 && U == 1), "the tail of the vertex launch is the single-workgroup edge step");
    double mu_scale;
    if constexpr (P::TAIL) mu_scale = pre.mu_scale;      // (the launch has already found the status RUNNING)
    else {
        if (cb->status != GCSADMM_RUNNING) return;
        mu_scale = cb->mu_scale;
    }
    double s[5] = {0, 0, 0, 0, 0};
    // a workgroup takes tiles of U x EDGE_BLOCK consecutive edges; a thread handles U edges of the tile, EDGE_BLOCK apart, and issues
    // the loads of all of them before the first use: U x 5C coalesced 4/8-byte loads in flight per thread (one edge per thread left
    // the stream latency-bound: 64 MB in 36 us on the 100k lattice)
    if constexpr (P::TAIL) {
        // one edge per thread, loaded CH words at a time (tail_words: the registers of the kernel this is the tail of); the words are
        // taken in the order of the loop below, so the five sums are accumulated in the same order
        constexpr int CH = tail_words<T, C>();
        const int e = (int)threadIdx.x;
        if (P::edge_thread() && e < a.E) {
            const int it = pre.it, ih = pre.ih;
            const double we = a.edge_counted ? (double)a.edge_counted[e] : 1.0;
            const double wt = a.inc_counted ? (double)a.inc_counted[it] : 1.0;
            const double wh = a.inc_counted ? (double)a.inc_counted[ih] : 1.0;
#pragma unroll
            for (int w0 = 0; w0 < C; w0 += CH) {
                T cu_[CH], cw_[CH], zo_[CH], mu_[CH], mw_[CH];
#pragma unroll
                for (int j = 0; j < CH; ++j) {
                    const int w = w0 + j;
                    if (w >= C) break;
                    cu_[j] = P::load_copy(&a.copy[(size_t)w * a.NI + it]); cw_[j] = P::load_copy(&a.copy[(size_t)w * a.NI + ih]);
                    zo_[j] = a.zedge[(size_t)w * a.E + e];
                    mu_[j] = a.mu[(size_t)w * a.NI + it]; mw_[j] = a.mu[(size_t)w * a.NI + ih];
                }
#pragma unroll
                for (int j = 0; j < CH; ++j) {
                    const int w = w0 + j;
                    if (w >= C) break;
                    edge_word(a, w, e, it, ih, cu_[j], cw_[j], zo_[j], mu_[j], mw_[j], mu_scale, we, wt, wh, s);
                }
            }
        }
    } else
    for (int base = bx * (U * EDGE_BLOCK); base < a.E; base += nblocks * (U * EDGE_BLOCK)) {
        int it[U], ih[U];
        T cu_[U][C], cw_[U][C], zo_[U][C], mu_[U][C], mw_[U][C];
#pragma unroll
        for (int q = 0; q < U; ++q) {
            const int e = base + q * EDGE_BLOCK + (int)threadIdx.x, ee = e < a.E ? e : a.E - 1;     // (tail of the last tile: a valid edge, result unused)
            // edge-major columns (null index arrays): the two columns of edge e are e and E + e, every access below is a stream
            it[q] = a.edge_inc_tail ? a.edge_inc_tail[ee] : ee; ih[q] = a.edge_inc_head ? a.edge_inc_head[ee] : a.E + ee;
#pragma unroll
            for (int w = 0; w < C; ++w) {
                cu_[q][w] = a.copy[(size_t)w * a.NI + it[q]]; cw_[q][w] = a.copy[(size_t)w * a.NI + ih[q]];
                zo_[q][w] = a.zedge[(size_t)w * a.E + ee];
                mu_[q][w] = a.mu[(size_t)w * a.NI + it[q]]; mw_[q][w] = a.mu[(size_t)w * a.NI + ih[q]];
            }
        }
#pragma unroll
        for (int q = 0; q < U; ++q) {
            const int e = base + q * EDGE_BLOCK + (int)threadIdx.x;
            if (e >= a.E) break;
            const double we = a.edge_counted ? (double)a.edge_counted[e] : 1.0;
            const double wt = a.inc_counted ? (double)a.inc_counted[it[q]] : 1.0;
            const double wh = a.inc_counted ? (double)a.inc_counted[ih[q]] : 1.0;
#pragma unroll
            for (int w = 0; w < C; ++w)
                edge_word(a, w, e, it[q], ih[q], cu_[q][w], cw_[q][w], zo_[q][w], mu_[q][w], mw_[q][w], mu_scale, we, wt, wh, s);
        }
    }
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
#pragma unroll
    for (int k = 0; k < 5; ++k) {
        const double t = wave_sum(s[k]);
        if (lane == 0 && P::edge_thread()) red[wv][k] = t;
    }
    P::sync();
    if (threadIdx.x < 5) {
        double t = 0;
        for (int q = 0; q < EDGE_BLOCK / EDGE_WAVE; ++q) t += red[q][threadIdx.x];
        if (MODE >= 2) __hip_atomic_store(&a.partials[(size_t)bx * 5 + threadIdx.x], t, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        else a.partials[(size_t)bx * 5 + threadIdx.x] = t;
        if (MODE == 1) sums[threadIdx.x] = t;      // one workgroup: its partial is the sum (what finalize_kernel would produce)
        if constexpr (P::TAIL) red[0][threadIdx.x] = t;      // (thread k has read column k of red, and nobody else does)
    }
    if (MODE == 1) {
        P::sync();
        if (threadIdx.x == 0) control_body<P>(cb, P::TAIL ? &red[0][0] : sums, cp, counters, trace);
    }
    if (MODE >= 2) {
        // hand-off of the partials to the last workgroup (MI355X_MICROARCH.md, inter-workgroup visibility): write-through (sc1)
        // stores by the first wavefront, drained, then ONE agent-scope ticket add by a lane of that same wavefront; the
        // workgroup whose add returns nblocks - 1 came last and reads every partial with sc1 loads.  (Measured alternative: an
        // agent-scope ACQ_REL ticket add instead of the drain -- the release writes back the L2 of the XCD, which holds this
        // kernel's own 24 MB of stores: edge step 23.6 -> 33.4 us on the 100k lattice.  Only the five partials need to cross.)
        if (threadIdx.x < EDGE_WAVE) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        if (threadIdx.x == 0) {
            const unsigned t = __hip_atomic_fetch_add(ticket, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            *is_last = (t == nblocks - 1);
        }
        __syncthreads();
        if (!*is_last) return;
        double acc[5] = {0, 0, 0, 0, 0};
        for (int b = threadIdx.x; b < (int)nblocks; b += EDGE_BLOCK)
            for (int k = 0; k < 5; ++k) acc[k] += __hip_atomic_load(&a.partials[(size_t)b * 5 + k], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        __syncthreads();       // red[][] above has been consumed by every thread
        for (int k = 0; k < 5; ++k) red[threadIdx.x][k] = acc[k];
        __syncthreads();
        for (int off = EDGE_BLOCK / 2; off > 0; off >>= 1) {
            if ((int)threadIdx.x < off)
                for (int k = 0; k < 5; ++k) red[threadIdx.x][k] += red[threadIdx.x + off][k];
            __syncthreads();
        }
        if (threadIdx.x < 5) sums[threadIdx.x] = red[0][threadIdx.x];
        __syncthreads();
        if (threadIdx.x == 0) {
            if (MODE == 2) control_body(cb, sums, cp, counters, trace);
            else sums[5] = (double)counters[0];
            __hip_atomic_store(ticket, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);     // ready for the next launch
        }
    }
}

}  // namespace gcsadmm_k
