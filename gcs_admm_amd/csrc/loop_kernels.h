// loop_kernels.h -- the __global__ kernels of the iteration loop's object (gcsadmm.hip, which has the list and the host side): edge and
// control steps, the batch forms, the slowest-first reorder, the final reduction, the halo pack / unpack and the cost.  In the
// anonymous namespace of the one translation unit that includes it.
#pragma once
#include <hip/hip_runtime.h>

#include "gcsadmm.h"
#include "edge_step.h"
#include "state_transfer_core.h"

namespace {

using namespace gcs;
using namespace gcsadmm_k;

// -------------------------------------------------------------------------------------------------
// edge and control kernels: the bodies are edge_step.h's (EdgeArgs<T>, ControlParams, edge_body<T, MODE, C, U>, control_body)
// -------------------------------------------------------------------------------------------------
__global__ void control_kernel(gcsadmm_control_block *cb, const double *sums, ControlParams p, int *counters, double *trace, bool global_fails)
{
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    control_body(cb, sums, p, counters, trace, global_fails);
}

template <class T, int MODE, int C, int U>
__global__ __launch_bounds__(EDGE_BLOCK) void edge_kernel(EdgeArgs<T> a, gcsadmm_control_block *cb, double *sums, ControlParams cp,
                                                          int *counters, double *trace, unsigned *ticket)
{
    __shared__ double red[EDGE_BLOCK][5];
    __shared__ int is_last;
    edge_body<T, MODE, C, U>(a, cb, sums, cp, counters, trace, ticket, blockIdx.x, gridDim.x, red, &is_last);
}

// BATCH form (gcsadmm_batch_run): row blockIdx.y of the grid is member blockIdx.y of the batch.  The workgroup copies that member's entry
// of the table -- what edge_kernel gets in its kernarg segment, plus the member's own number of workgroups -- through a uniform index
// (scalar loads) and runs the body in the mode gcsadmm_run uses for that member: MODE 1 where one workgroup
// holds all its edges, MODE 2 otherwise, with the member's nblocks in place of gridDim.x in the edge loop, the partials and the ticket
// (each member has its own partials, sums, counters and ticket: its handle's).  The grid is as wide as the widest member; the
// workgroups beyond a member's own leave before they touch its ticket or partials.  One edge per thread (U = 1: batch_plan.h).
template <class T> struct EdgeBatchEntry {
    EdgeArgs<T> a;
    gcsadmm_control_block *cb;
    double *sums;
    ControlParams cp;
    int *counters;
    double *trace;      // may be null
    unsigned *ticket;
    int nblocks;
};
template <class T, int C>
__global__ __launch_bounds__(EDGE_BLOCK) void edge_batch_kernel(const EdgeBatchEntry<T> *__restrict__ table)
{
    __shared__ double red[EDGE_BLOCK][5];
    __shared__ int is_last;
    // (read through the constant address space, as kernel arguments are: vertex_wg_batch_kernel has the reason)
    __builtin_assume_dereferenceable(table + blockIdx.y, sizeof(EdgeBatchEntry<T>));
    const EdgeBatchEntry<T> e = *(const EdgeBatchEntry<T> *)((const __attribute__((address_space(4))) EdgeBatchEntry<T> *)table + blockIdx.y);
    if ((int)blockIdx.x >= e.nblocks) return;
    if (e.nblocks == 1) edge_body<T, 1, C, 1>(e.a, e.cb, e.sums, e.cp, e.counters, e.trace, e.ticket, 0, 1, red, &is_last);
    else edge_body<T, 2, C, 1>(e.a, e.cb, e.sums, e.cp, e.counters, e.trace, e.ticket, blockIdx.x, (unsigned)e.nblocks, red, &is_last);
}

// status and it of the members' control blocks, gathered for the one copy of gcsadmm_batch_poll: out[i] = status, out[count + i] = it
__global__ __launch_bounds__(256) void batch_poll_kernel(const gcsadmm_control_block *const *cbs, int count, int *out)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= count) return;
    out[i] = cbs[i]->status;
    out[count + i] = cbs[i]->it;
}

// STATE TRANSFER (gcsadmm_export_state / gcsadmm_import_state and their batch forms): the bodies are state_transfer_core.h's.  One launch
// for all members of a call; a workgroup finds its member in the table's prefix of workgroup counts (uniform per workgroup) and runs
// the lanes of one tile of that member's edges or, in the member's trailing workgroups, vertices.
template <class T>
__global__ __launch_bounds__(TRANSFER_BLOCK) void state_export_kernel(const TransferEntry *__restrict__ table, int count)
{
    const TransferEntry e = table[transfer_member(table, count, (int)blockIdx.x)];
    transfer_export_lane<T>(e, (int)blockIdx.x - e.block_first, (int)threadIdx.x);
}
template <class T>
__global__ __launch_bounds__(TRANSFER_BLOCK) void state_import_kernel(const TransferEntry *__restrict__ table, int count)
{
    const TransferEntry e = table[transfer_member(table, count, (int)blockIdx.x)];
    transfer_import_lane<T>(e, (int)blockIdx.x - e.block_first, (int)threadIdx.x);
}

// SLOWEST-FIRST DISPATCH.  A vertex-step launch ends when its slowest workgroup does, and with the warm start most solves take 3-5
// Newton iterations while a few take 15: on the 10k lattice (1 654 wavefronts on 1 024 one-wavefront-per-SIMD slots) a slow
// wavefront that happens to start in the second round ends the launch at 21 iteration times instead of 17.  Every few ADMM
// iterations the units (wavefronts / workgroups) are re-ordered by the Newton iterations of their last launch, descending: a
// counting sort by one workgroup.  The order among equal counts is arbitrary (atomics); it affects scheduling only, never results.
constexpr int REORDER_BINS = 64, REORDER_THREADS = 1024, REORDER_EVERY = 8;     // (REORDER_MIN_UNITS: create_plan.h)
// ids (may be null): the units to order are ids[0 .. n) instead of 0 .. n (the boundary / interior subsets of a partition's overlapped loop)
__global__ __launch_bounds__(REORDER_THREADS) void reorder_kernel(int n, const int *iters, int *order, const gcsadmm_control_block *cb, const int *ids = nullptr)
{
    if (cb->status != GCSADMM_RUNNING) return;
    __shared__ int cnt[REORDER_BINS], off[REORDER_BINS];
    if (threadIdx.x < REORDER_BINS) cnt[threadIdx.x] = 0;
    __syncthreads();
    auto unit = [&](int i) { return ids ? ids[i] : i; };
    auto key = [&](int i) { const int k = iters[unit(i)]; return k < 0 ? 0 : (k >= REORDER_BINS ? REORDER_BINS - 1 : k); };
    for (int i = threadIdx.x; i < n; i += REORDER_THREADS) atomicAdd(&cnt[key(i)], 1);
    __syncthreads();
    if (threadIdx.x == 0) {
        int run = 0;
        for (int b = REORDER_BINS - 1; b >= 0; --b) { off[b] = run; run += cnt[b]; }
    }
    __syncthreads();
    for (int i = threadIdx.x; i < n; i += REORDER_THREADS) order[atomicAdd(&off[key(i)], 1)] = unit(i);
}

// fixed-order reduction of the per-workgroup partials -> sums[5]
__global__ __launch_bounds__(256) void finalize_kernel(const double *partials, int nblocks, double *sums,
                                                      const gcsadmm_control_block *cb)
{
    if (cb->status != GCSADMM_RUNNING) return;
    __shared__ double red[256][5];
    double s[5] = {0, 0, 0, 0, 0};
    for (int b = threadIdx.x; b < nblocks; b += 256)
        for (int k = 0; k < 5; ++k) s[k] += partials[(size_t)b * 5 + k];
    for (int k = 0; k < 5; ++k) red[threadIdx.x][k] = s[k];
    __syncthreads();
    for (int off = 128; off > 0; off >>= 1) {
        if ((int)threadIdx.x < off)
            for (int k = 0; k < 5; ++k) red[threadIdx.x][k] += red[threadIdx.x + off][k];
        __syncthreads();
    }
    if (threadIdx.x < 5) sums[threadIdx.x] = red[0][threadIdx.x];
}

// halo of a vertex partition: copies of the cut edges' coupled words, packed per neighbour as [c][columns of that peer]
// (one contiguous message per peer).  base[j] / stride[j]: where column j of the flat send (recv) list sits in the buffer.
template <class T>
__global__ __launch_bounds__(256) void halo_pack_kernel(int c, int ncols, int NI, const int *cols, const int *base, const int *stride,
                                                        const T *copy, T *buf, const gcsadmm_control_block *cb)
{
    if (cb->status != GCSADMM_RUNNING) return;
    const int t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= c * ncols) return;
    const int w = t / ncols, j = t - w * ncols;
    buf[base[j] + w * stride[j]] = copy[(size_t)w * NI + cols[j]];
}
template <class T>
__global__ __launch_bounds__(256) void halo_unpack_kernel(int c, int ncols, int NI, const int *cols, const int *base, const int *stride,
                                                          const T *buf, T *copy, const gcsadmm_control_block *cb)
{
    if (cb->status != GCSADMM_RUNNING) return;
    const int t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= c * ncols) return;
    const int w = t / ncols, j = t - w * ncols;
    copy[(size_t)w * NI + cols[j]] = buf[base[j] + w * stride[j]];
}
template <class T>
__global__ __launch_bounds__(256) void cost_kernel(int V, int E, int n, const double *zv, const T *zedge,
                                                   const uint8_t *edge_counted, double eps_edge, double *cost)
{
    // single workgroup, fixed order: this runs once after the loop
    __shared__ double red[256];
    double s = 0;
    for (int v = threadIdx.x; v < V; v += 256) {
        double q = 0;
        for (int k = 0; k < n; ++k) { const double dlt = zv[(size_t)v * 2 * n + k] - zv[(size_t)v * 2 * n + n + k]; q += dlt * dlt; }
        s += sqrt(q);
    }
    for (int e = threadIdx.x; e < E; e += 256)
        s += eps_edge * (edge_counted ? (double)edge_counted[e] : 1.0) * (double)zedge[(size_t)(2 * n) * E + e];
    red[threadIdx.x] = s;
    __syncthreads();
    for (int off = 128; off > 0; off >>= 1) {
        if ((int)threadIdx.x < off) red[threadIdx.x] += red[threadIdx.x + off];
        __syncthreads();
    }
    if (threadIdx.x == 0) cost[0] = red[0];
}


} // namespace
