// gcsadmm.hip -- gfx950 kernels and C ABI (include/gcsadmm.h) of the ADMM iteration loop.
//
// Kernels (one HIP stream, launched back to back, no host round trip inside the loop):
//   vertex_kernel<2,T>   x-update, wavefront program (n = 2, degree <= 63): one wavefront per workgroup, several vertices
//                        per wavefront, program in vertex_program.h     (admm_solver_v3.py:352-540)
//   vertex_wg_kernel<N,T> (vertex_wg.hip) x-update, workgroup program: one 256-thread workgroup per vertex, any n / degree
//                        trailing workgroups of either launch: x-update of s, t (closed form) and of vertices no flow can cross
//   vertex_wg_split_kernel<N,T> (vertex_wg.hip) the same program for vertices too large for LDS, edge blocks in a device workspace
//   edge_kernel<T,MODE,C> z-update, dual update, five partial norms     (admm_solver_v3.py:543-614); in gcsadmm_run the last
//                        workgroup to finish also does the final reduction and the control step (one launch per edge step)
//   finalize_kernel / control_kernel   deterministic final reduction; residuals, rho adaptation, stop test,
//                        trace record (admm_solver_v3.py:697-733): the separate steps of the partitioned loop
//   halo_pack / halo_unpack_kernel     messages of the cut edges' copies between vertex partitions (RCCL); in the overlapped
//                        partitioned loop they and the transfer run on a second stream while the interior wavefronts are solved
//   cost_kernel<T>       GCS_utils.py:184-211
#include <hip/hip_runtime.h>
#include <dlfcn.h>
#include <rccl/rccl.h>

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <new>
#include <string>
#include <type_traits>
#include <vector>

#include "gcsadmm.h"
#include "terminal_launch.h"
#ifdef GCS_PHASE_TIMING
// diagnostic build: sub-phase stamps inside the border factorisation (lane 0 of each wavefront)
__device__ unsigned long long g_sub_cycles[16];
__device__ __forceinline__ void gcs_stamp(int k)
{
    static __shared__ unsigned long long last;
    __builtin_amdgcn_sched_barrier(0);
    if (threadIdx.x == 0) {
        const unsigned long long t = __builtin_amdgcn_s_memtime();
        if (k > 0) atomicAdd(&g_sub_cycles[k], t - last);
        last = t;
    }
    __builtin_amdgcn_sched_barrier(0);
}
#define GCS_STAMP(k) gcs_stamp(k)
#endif
#include "vertex_kernel.h"
#include "vertex_wg_launch.h"
#include "warm_start.h"
#include "canonical_box.h"
#include "create_plan.h"

namespace {

using namespace gcs;
using namespace gcsadmm_k;

// -------------------------------------------------------------------------------------------------
// edge kernel: one thread per directed edge, all c coupled words
// -------------------------------------------------------------------------------------------------
template <class T> struct EdgeArgs {
    int E, NI, c;
    const int *edge_inc_tail, *edge_inc_head;
    const uint8_t *inc_counted, *edge_counted;   // may be null
    const T *copy;
    T *zedge, *mu;
    double *partials;    // [gridDim.x][5]
};

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

// admm_solver_v3.py:697-733 on the five (globally reduced) sums; one thread
// global_fails: the inner-failure count comes with the (all-reduced) sums as sums[5] instead of from this handle's counter
__device__ void control_body(gcsadmm_control_block *cb, const double *sums, const ControlParams &p, int *counters, double *trace,
                             bool global_fails = false)
{
    if (cb->status != GCSADMM_RUNNING) return;
    double s[5];
    for (int k = 0; k < 5; ++k) { s[k] = sums[k]; cb->sums[k] = s[k]; }
    const int it = cb->it;
    double rho = cb->rho;
    const int fails = global_fails ? (int)(sums[5] + 0.5) : counters[0], iters = counters[1];
    counters[0] = 0; counters[1] = 0;
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

__global__ void control_kernel(gcsadmm_control_block *cb, const double *sums, ControlParams p, int *counters, double *trace, bool global_fails)
{
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    control_body(cb, sums, p, counters, trace, global_fails);
}

// edges a thread of the edge kernel has in flight at once on LARGE graphs (registers: U x 5C words); which graphs use it:
// edge_unroll_rt (create_plan.h)
template <class T, int C> __host__ __device__ constexpr int edge_unroll() { return sizeof(T) == 4 ? (C <= 7 ? 4 : 2) : (C <= 7 ? 2 : 1); }

// MODE 0: partial sums per workgroup only (gcsadmm_edge_step: the caller all-reduces / finalizes);
// MODE 1: single workgroup (at most EDGE_BLOCK edges, gcsadmm_run on small graphs): the workgroup also does the final
//         reduction and the control step;
// MODE 2: any grid (gcsadmm_run): the LAST workgroup to finish -- told by an agent-scope ticket counter -- reduces all the
//         partials in the fixed order of finalize_kernel and runs the control step: one launch per edge step instead of two;
// MODE 3: as MODE 2 without the control step (gcsadmm_run_partitioned): the last workgroup leaves the five sums and, in
//         sums[5], this partition's inner-failure count for the all-reduce that follows.
// C = coupled words per copy (2n+1), compile-time so that all C x 5 loads of an edge are in flight at once.
template <class T, int MODE, int C, int U>
__global__ __launch_bounds__(EDGE_BLOCK) void edge_kernel(EdgeArgs<T> a, gcsadmm_control_block *cb, double *sums, ControlParams cp,
                                                          int *counters, double *trace, unsigned *ticket)
{
    if (cb->status != GCSADMM_RUNNING) return;
    const double mu_scale = cb->mu_scale;
    double s[5] = {0, 0, 0, 0, 0};
    // a workgroup takes tiles of U x EDGE_BLOCK consecutive edges; a thread handles U edges of the tile, EDGE_BLOCK apart, and issues
    // the loads of all of them before the first use: U x 5C coalesced 4/8-byte loads in flight per thread (one edge per thread left
    // the stream latency-bound: 64 MB in 36 us on the 100k lattice)
    for (int base = blockIdx.x * (U * EDGE_BLOCK); base < a.E; base += gridDim.x * (U * EDGE_BLOCK)) {
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
            for (int w = 0; w < C; ++w) {
                const double cu = (double)cu_[q][w], cw = (double)cw_[q][w], zo = (double)zo_[q][w];
                const T zn_t = (T)(0.5 * (cu + cw));
                const double zn = (double)zn_t;
                const double ru = cu - zn, rw = cw - zn;
                const T mu_u_t = (T)scaled_plus(mu_scale, (double)mu_[q][w], ru);
                const T mu_w_t = (T)scaled_plus(mu_scale, (double)mw_[q][w], rw);
                a.mu[(size_t)w * a.NI + it[q]] = mu_u_t;
                a.mu[(size_t)w * a.NI + ih[q]] = mu_w_t;
                a.zedge[(size_t)w * a.E + e] = zn_t;
                const double mu_u = (double)mu_u_t, mu_w = (double)mu_w_t;
                s[0] += wt * ru * ru + wh * rw * rw;
                s[1] += we * (zn - zo) * (zn - zo);
                s[2] += wt * cu * cu + wh * cw * cw;
                s[3] += we * zn * zn;
                s[4] += wt * mu_u * mu_u + wh * mu_w * mu_w;
            }
        }
    }
    __shared__ double red[EDGE_BLOCK][5];
    __shared__ int is_last;
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
#pragma unroll
    for (int k = 0; k < 5; ++k) {
        const double t = wave_sum(s[k]);
        if (lane == 0) red[wv][k] = t;
    }
    __syncthreads();
    if (threadIdx.x < 5) {
        double t = 0;
        for (int q = 0; q < EDGE_BLOCK / WAVE; ++q) t += red[q][threadIdx.x];
        if (MODE >= 2) __hip_atomic_store(&a.partials[(size_t)blockIdx.x * 5 + threadIdx.x], t, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        else a.partials[(size_t)blockIdx.x * 5 + threadIdx.x] = t;
        if (MODE == 1) sums[threadIdx.x] = t;      // one workgroup: its partial is the sum (what finalize_kernel would produce)
    }
    if (MODE == 1) {
        __syncthreads();
        if (threadIdx.x == 0) control_body(cb, sums, cp, counters, trace);
    }
    if (MODE >= 2) {
        // hand-off of the partials to the last workgroup (MI355X_MICROARCH.md, inter-workgroup visibility): write-through (sc1)
        // stores by the first wavefront, drained, then ONE agent-scope ticket add by a lane of that same wavefront; the
        // workgroup whose add returns gridDim.x - 1 came last and reads every partial with sc1 loads.  (Measured alternative: an
        // agent-scope ACQ_REL ticket add instead of the drain -- the release writes back the L2 of the XCD, which holds this
        // kernel's own 24 MB of stores: edge step 23.6 -> 33.4 us on the 100k lattice.  Only the five partials need to cross.)
        if (threadIdx.x < WAVE) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        if (threadIdx.x == 0) {
            const unsigned t = __hip_atomic_fetch_add(ticket, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            is_last = (t == gridDim.x - 1);
        }
        __syncthreads();
        if (!is_last) return;
        const int nblocks = gridDim.x;
        double acc[5] = {0, 0, 0, 0, 0};
        for (int b = threadIdx.x; b < nblocks; b += EDGE_BLOCK)
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

// =================================================================================================
// host side
// =================================================================================================
struct gcsadmm_handle_s {
    int n = 0, V = 0, E = 0, NI = 0, NI_owned = 0, c = 0, MM = 0, dtype = 0, device = 0;
    int n_waves = 0, n_special = 0, slots_cap = 0, lds_bytes = 0, edge_blocks = 0;
    int n_wg = 0, wg_lds_bytes = 0;   // vertices solved by the workgroup program (vertex_wg.hip), LDS per workgroup
    int wg_box = 0;           // every workgroup-program vertex is a canonical box: BOX instantiation of that program
    int wg_t512 = 0;          // the launch uses the 512-thread build of the workgroup program (at most one workgroup per CU)
    // split form of the workgroup program (gcsadmm_graph_desc.vertex_workspace): vertices, LDS per workgroup, their units' slabs
    int n_split = 0, split_lds_bytes = 0;
    int *d_split_vtx = nullptr;
    long long *d_split_off = nullptr;
    double *d_split_ws = nullptr;
    size_t split_doubles = 0;
    int edge_unroll = 1;      // edges in flight per thread of the edge kernel
    int edge_major = 0;       // state columns numbered by edge (gcsadmm_graph_desc.edge_major_columns)
    std::vector<char> col_owned;   // [NI] 1: the column of an incidence of this handle's vertices, 0: a ghost column
    int all_m4 = 0;           // 2: every wavefront-program vertex is a canonical box (4 facets) -> the box instantiation; 0: the generic one
    int align_rows = 0;       // group placement rule (group_base)
    int store_dl = 0;         // LDS holds the final dual directions of the facet rows (kernel template SDL)
    double nx = 0, nmu = 0;
    gcsadmm_params params{};
    bool params_set = false;
    // device buffers
    int *d_inc_ptr = nullptr, *d_deg_in = nullptr, *d_inc_edge = nullptr, *d_poly_ptr = nullptr;
    int *d_edge_inc_tail = nullptr, *d_edge_inc_head = nullptr;
    int *d_wave_slot_ptr = nullptr, *d_wave_vtx = nullptr, *d_special_vtx = nullptr, *d_special_kind = nullptr, *d_wg_vtx = nullptr;
    double *d_poly_A = nullptr, *d_poly_bc = nullptr, *d_center = nullptr;
    uint8_t *d_inc_counted = nullptr, *d_edge_counted = nullptr;
    gcsadmm_control_block *d_cb = nullptr;
    int *d_counters = nullptr;
    double *d_partials = nullptr, *d_sums = nullptr;
    unsigned *d_ticket = nullptr;
    // prox configuration (gcsadmm_vertex_prox): every non-terminal vertex, LDS of the border-only problem, own counters
    int *d_prox_vtx = nullptr, *d_prox_counters = nullptr, n_prox = 0, prox_lds_bytes = 0, src = -1, dst = -1;     // arrival counter of the single-launch edge step (edge_kernel MODE 2)
    std::vector<hipEvent_t> events;
    std::string err;
    // vertex partition across GPUs (gcsadmm_attach_comm): RCCL communicator, halo index lists and message buffers
    void *comm = nullptr;             // ncclComm_t
    int rank = 0, world = 1;
    std::vector<int> peers, peer_cnt, peer_off;   // neighbour ranks; columns per peer; first column of each peer's block
    int n_send = 0, n_recv = 0;       // halo columns sent / received per iteration
    int *d_send_cols = nullptr, *d_send_base = nullptr, *d_send_stride = nullptr;
    int *d_recv_cols = nullptr, *d_recv_base = nullptr, *d_recv_stride = nullptr;
    void *d_sendbuf = nullptr, *d_recvbuf = nullptr;
    double *d_sums6 = nullptr;        // the five norms + the inner-failure count, all-reduced together
    // warm start of the vertex solves (warm_start.h): one record per generic vertex, d_warm + d_warm_ptr[v]
    double *d_warm = nullptr;
    long long *d_warm_ptr = nullptr;
    size_t warm_doubles = 0;
    // slowest-first dispatch (reorder_kernel): per wavefront / per workgroup-program vertex, last Newton iteration count and launch order
    int *d_wave_iters = nullptr, *d_wave_order = nullptr, *d_wg_iters = nullptr, *d_wg_order = nullptr;
    int vertex_steps = 0;     // vertex steps enqueued since the last reset
    // overlapped partitioned loop (boundary vertices first, the halo exchange behind them while the interior is solved):
    // host copies of the wavefront packing (which wavefront holds which vertex) and of the column -> vertex map, the split of the
    // wavefronts into boundary (holding a vertex with a cut edge) and interior, a second stream for the exchange and two events
    std::vector<int> h_wave_slot_ptr, h_wave_vtx, col_vertex;
    int overlap_mode = 0;     // gcsadmm_set_overlap: 0 automatic, 1 forced (tests: works without peers), 2 off
    int n_wave_b = 0;         // boundary wavefronts (0: no split)
    int *d_split_ids = nullptr, *d_split_order = nullptr;    // [n_waves] static ids / launch order: boundary wavefronts first, then interior
    hipStream_t comm_stream = nullptr;
    hipEvent_t ev_boundary = nullptr, ev_halo = nullptr;
    // terminals that are regions (terminal_region.h): at most two, one workgroup each, on an auxiliary stream beside the vertex-step launch
    int n_term = 0, term_vtx[2] = {-1, -1}, term_is_src[2] = {0, 0};
    long long term_ws_off[2] = {0, 0}, term_rec_off[2] = {0, 0};
    double *d_term_ws = nullptr, *d_term_rec = nullptr;      // work arrays (when they do not fit LDS); warm-start records
    size_t term_rec_doubles = 0;
    int term_threads = 256, term_lds_doubles = 0;     // launch shape: one wavefront and LDS work arrays for small terminals
    hipStream_t term_stream = nullptr;
    hipEvent_t ev_term_fork = nullptr, ev_term_join = nullptr;
};

// ---- RCCL, bound at run time ----
// The library is not linked against librccl: a process that already carries an RCCL (PyTorch-ROCm ships its own copy with the
// SONAME of /opt/rocm's) must not end up with two, and a single-GPU user needs none.  dlopen returns the copy that is already
// loaded, or loads the system one.
namespace {
struct RcclApi {
    void *lib = nullptr;
    decltype(&ncclGetUniqueId) GetUniqueId = nullptr;
    decltype(&ncclCommInitRank) CommInitRank = nullptr;
    decltype(&ncclCommDestroy) CommDestroy = nullptr;
    decltype(&ncclGroupStart) GroupStart = nullptr;
    decltype(&ncclGroupEnd) GroupEnd = nullptr;
    decltype(&ncclSend) Send = nullptr;
    decltype(&ncclRecv) Recv = nullptr;
    decltype(&ncclAllReduce) AllReduce = nullptr;
    decltype(&ncclGetErrorString) GetErrorString = nullptr;
    decltype(&ncclCommCount) CommCount = nullptr;
    std::string err;
    bool ok() const { return lib && GetUniqueId && CommInitRank && CommDestroy && GroupStart && GroupEnd && Send && Recv && AllReduce; }
};
RcclApi &rccl()
{
    static RcclApi api = [] {
        RcclApi a;
        for (const char *name : {"librccl.so.1", "librccl.so"}) {
            a.lib = dlopen(name, RTLD_NOW | RTLD_GLOBAL);
            if (a.lib) break;
        }
        if (!a.lib) {
            const char *why = dlerror();      // (a second call would return NULL: the message is consumed)
            a.err = std::string("dlopen(librccl): ") + (why ? why : "not found");
            return a;
        }
#define RCCL_SYM(f) a.f = (decltype(a.f))dlsym(a.lib, "nccl" #f)
        RCCL_SYM(GetUniqueId); RCCL_SYM(CommInitRank); RCCL_SYM(CommDestroy); RCCL_SYM(GroupStart); RCCL_SYM(GroupEnd);
        RCCL_SYM(Send); RCCL_SYM(Recv); RCCL_SYM(AllReduce); RCCL_SYM(GetErrorString); RCCL_SYM(CommCount);
#undef RCCL_SYM
        if (!a.ok()) a.err = "librccl lacks an expected symbol";
        return a;
    }();
    return api;
}
}  // namespace
#define NCCLCHK(h, call)                                                                             \
    do {                                                                                             \
        ncclResult_t r_ = (call);                                                                    \
        if (r_ != ncclSuccess) {                                                                     \
            (h)->err = std::string(#call) + ": " + (rccl().GetErrorString ? rccl().GetErrorString(r_) : "RCCL error"); \
            return GCSADMM_ERR_HIP;                                                                  \
        }                                                                                            \
    } while (0)


static std::string g_create_error;

// Entry points work on the handle's device and leave the caller's current device as they found it (a process may hold
// handles on several devices, and PyTorch tracks "its" current device on its own).
struct DeviceGuard {
    int prev = -1;
    hipError_t err = hipSuccess;
    explicit DeviceGuard(int dev)
    {
        int cur = -1;
        err = hipGetDevice(&cur);
        if (err == hipSuccess && cur != dev) { err = hipSetDevice(dev); if (err == hipSuccess) prev = cur; }
    }
    ~DeviceGuard() { if (prev >= 0) (void)hipSetDevice(prev); }
    DeviceGuard(const DeviceGuard &) = delete;
    DeviceGuard &operator=(const DeviceGuard &) = delete;
};
#define USE_DEVICE(h)                                                                                \
    DeviceGuard device_guard_((h)->device);                                                          \
    do {                                                                                             \
        if (device_guard_.err != hipSuccess) {                                                       \
            (h)->err = std::string("hipSetDevice: ") + hipGetErrorString(device_guard_.err);        \
            return GCSADMM_ERR_HIP;                                                                  \
        }                                                                                            \
    } while (0)

#define HIPCHK(h, call)                                                                              \
    do {                                                                                             \
        hipError_t e_ = (call);                                                                      \
        if (e_ != hipSuccess) {                                                                      \
            (h)->err = std::string(#call) + ": " + hipGetErrorString(e_);                            \
            return GCSADMM_ERR_HIP;                                                                  \
        }                                                                                            \
    } while (0)

template <class U> static hipError_t upload(U **dst, const U *src, size_t count)
{
    *dst = nullptr;
    if (count == 0) count = 1;
    hipError_t e = hipMalloc((void **)dst, count * sizeof(U));
    if (e != hipSuccess) return e;
    if (src) return hipMemcpy(*dst, src, count * sizeof(U), hipMemcpyHostToDevice);
    return hipMemset(*dst, 0, count * sizeof(U));
}

static VertexLaunchDesc make_launch_desc(gcsadmm_handle h, const gcsadmm_state *st);
static void halo_free(gcsadmm_handle h);

// the inputs every vertex-step launch shares (step_args.h)
static StepDesc make_step(gcsadmm_handle h, const gcsadmm_state *st)
{
    StepDesc a;
    a.inc_ptr = h->d_inc_ptr; a.deg_in = h->d_deg_in; a.inc_edge = h->d_inc_edge; a.poly_ptr = h->d_poly_ptr;
    a.poly_A = h->d_poly_A; a.poly_bc = h->d_poly_bc; a.center = h->d_center;
    a.E = h->E; a.NI = h->NI; a.edge_major = h->edge_major;
    a.zedge = st->zedge; a.mu = st->mu; a.copy = st->copy; a.xv = st->xv; a.zv = st->zv; a.yv = st->yv;
    a.counters = h->d_counters; a.cb = h->d_cb;
    a.eps_edge = h->params.eps_edge; a.ipm_tol = h->params.ipm_tol; a.ipm_max_iter = h->params.ipm_max_iter;
    a.warm = h->params.cold_start ? nullptr : h->d_warm; a.warm_ptr = h->d_warm_ptr;
    return a;
}

// The generic vertices of a handle are split at create between the wavefront program (n = 2, degree <= 63: vertex_kernel.h)
// and the workgroup program (everything else, and all vertices of small graphs: vertex_wg.hip); the closed-form vertices
// ride in the trailing workgroups of whichever launch exists.
static WgLaunchDesc make_wg_desc(gcsadmm_handle h, const gcsadmm_state *st, bool with_special)
{
    WgLaunchDesc d;
    d.step = make_step(h, st);
    d.n = h->n; d.dtype = h->dtype; d.n_vtx = h->n_wg; d.n_special = with_special ? h->n_special : 0; d.lds_bytes = h->wg_lds_bytes;
    d.vtx = h->d_wg_vtx; d.special_vtx = h->d_special_vtx; d.special_kind = h->d_special_kind; d.box = h->wg_box;
    d.order = h->d_wg_order; d.unit_iters = h->d_wg_iters;
    return d;
}

// part: -1 the whole vertex step; 0 / 1 the boundary / interior wavefronts of the overlapped partitioned loop (handles whose generic
// vertices are all on the wavefront program; the closed-form vertices ride with the boundary part)
static gcsadmm_k::TermLaunchDesc make_term_desc(gcsadmm_handle h, const gcsadmm_state *st)
{
    gcsadmm_k::TermLaunchDesc d;
    d.step = make_step(h, st);
    d.n = h->n; d.dtype = h->dtype; d.count = h->n_term; d.threads = h->term_threads; d.lds_doubles = h->term_lds_doubles;
    for (int i = 0; i < 2; ++i) {
        d.t.vtx[i] = h->term_vtx[i]; d.t.is_src[i] = h->term_is_src[i]; d.t.ws_off[i] = h->term_ws_off[i]; d.t.rec_off[i] = h->term_rec_off[i];
    }
    d.t.ws = h->d_term_ws;
    d.t.rec = h->params.cold_start ? nullptr : h->d_term_rec;
    return d;
}

template <class T> static gcsadmm_status launch_vertex(gcsadmm_handle h, const gcsadmm_state *st, hipStream_t s, int part = -1, bool reorder = false)
{
    // terminals that are regions: their kernel runs on the auxiliary stream beside the launches below (it is a latency-bound solve in
    // one or two workgroups; the vertex launches do not wait for it, the caller's stream does at the end)
    const bool with_term = h->n_term > 0 && part <= 0;
    if (with_term) {
        HIPCHK(h, hipEventRecord(h->ev_term_fork, s));
        HIPCHK(h, hipStreamWaitEvent(h->term_stream, h->ev_term_fork, 0));
        gcsadmm_terminal_launch(make_term_desc(h, st), h->term_stream);
        HIPCHK(h, hipEventRecord(h->ev_term_join, h->term_stream));
    }
    struct Join {       // (every return path below joins)
        gcsadmm_handle h; hipStream_t s; bool on;
        ~Join() { if (on) (void)hipStreamWaitEvent(s, h->ev_term_join, 0); }
    } join_{h, s, with_term};
    if (part >= 0) {
        VertexLaunchDesc d = make_launch_desc(h, st);
        const int off = part ? h->n_wave_b : 0, cnt = part ? h->n_waves - h->n_wave_b : h->n_wave_b;
        d.wave_order = h->d_split_order + off;
        d.n_waves = cnt;
        if (part) d.n_special = 0;
        launch_vertex_dim<2, T>(d, s);
        if (reorder && h->d_wave_iters)      // slowest first inside the part, on the part's own stream (its next launch reads the order)
            hipLaunchKernelGGL(reorder_kernel, dim3(1), dim3(REORDER_THREADS), 0, s, cnt, h->d_wave_iters, h->d_split_order + off, h->d_cb, h->d_split_ids + off);
        HIPCHK(h, hipGetLastError());
        return GCSADMM_OK;
    }
    const bool special_on_wave = h->n_waves > 0;
    if (h->n_waves > 0) {
        VertexLaunchDesc d = make_launch_desc(h, st);
        launch_vertex_dim<2, T>(d, s);
    }
    if (h->n_wg > 0 || (!special_on_wave && h->n_special > 0)) {
        if (h->wg_t512) gcsadmm_wg_launch_t512(make_wg_desc(h, st, !special_on_wave), s);
        else gcsadmm_wg_launch(make_wg_desc(h, st, !special_on_wave), s);
    }
    if (h->n_split > 0) {      // the vertices too large for LDS: the split form, units in the handle's workspace
        WgLaunchDesc d = make_wg_desc(h, st, false);
        d.n_vtx = h->n_split; d.vtx = h->d_split_vtx; d.lds_bytes = h->split_lds_bytes; d.order = nullptr; d.unit_iters = nullptr;
        gcsadmm_wg_launch_split(d, WgSplitArgs{h->d_split_ws, h->d_split_off}, s);
    }
    if (++h->vertex_steps % REORDER_EVERY == 0) {      // slowest-first dispatch of the following launches (graphs that need more than one round)
        if (h->d_wave_order) hipLaunchKernelGGL(reorder_kernel, dim3(1), dim3(REORDER_THREADS), 0, s, h->n_waves, h->d_wave_iters, h->d_wave_order, h->d_cb);
        if (h->d_wg_order) hipLaunchKernelGGL(reorder_kernel, dim3(1), dim3(REORDER_THREADS), 0, s, h->n_wg, h->d_wg_iters, h->d_wg_order, h->d_cb);
    }
    HIPCHK(h, hipGetLastError());
    return GCSADMM_OK;
}

// with_control: the control step rides in the same launches (gcsadmm_run); trace may be null
template <class T> static gcsadmm_status launch_edge(gcsadmm_handle h, const gcsadmm_state *st, double *sums, hipStream_t s,
                                                     bool with_control = false, double *trace = nullptr, bool sums6 = false)
{
    const gcsadmm_params &pp = h->params;
    const ControlParams cp{pp.tau_incr, pp.tau_decr, pp.nu, pp.eps_abs, pp.eps_rel, h->nx, h->nmu, pp.it_rho_limit, pp.max_it};
    EdgeArgs<T> a;
    a.E = h->E; a.NI = h->NI; a.c = h->c;
    a.edge_inc_tail = h->edge_major ? nullptr : h->d_edge_inc_tail; a.edge_inc_head = h->edge_major ? nullptr : h->d_edge_inc_head;
    a.inc_counted = h->d_inc_counted; a.edge_counted = h->d_edge_counted;
    a.copy = (const T *)st->copy; a.zedge = (T *)st->zedge; a.mu = (T *)st->mu; a.partials = h->d_partials;
    // one kernel instantiation per (state type, mode, words per copy)
    auto go = [&](auto mode, int blocks) {
        constexpr int M = decltype(mode)::value;
#define GCS_EDGE_U(CC, UU) hipLaunchKernelGGL((edge_kernel<T, M, CC, UU>), dim3(blocks), dim3(EDGE_BLOCK), 0, s, a, h->d_cb, sums, cp, h->d_counters, trace, h->d_ticket)
#define GCS_EDGE(CC) do { if (h->edge_unroll > 1) GCS_EDGE_U(CC, (edge_unroll<T, CC>())); else GCS_EDGE_U(CC, 1); } while (0)
        switch (h->c) {      // c = 2n + 1
        case 3: GCS_EDGE(3); break;
        case 5: GCS_EDGE(5); break;
        case 7: GCS_EDGE(7); break;
        case 9: GCS_EDGE(9); break;
        case 11: GCS_EDGE(11); break;
        case 13: GCS_EDGE(13); break;
        case 15: GCS_EDGE(15); break;
        default: GCS_EDGE(17);          // n = 8 (gcsadmm_create admits n = 1 .. 8)
        }
#undef GCS_EDGE_U
#undef GCS_EDGE
    };
    if (sums6) go(std::integral_constant<int, 3>(), h->edge_blocks);
    else if (with_control && h->edge_blocks == 1) go(std::integral_constant<int, 1>(), 1);
    else if (with_control) go(std::integral_constant<int, 2>(), h->edge_blocks);
    else {
        go(std::integral_constant<int, 0>(), h->edge_blocks);
        hipLaunchKernelGGL(finalize_kernel, dim3(1), dim3(256), 0, s, h->d_partials, h->edge_blocks, sums, h->d_cb);
    }
    HIPCHK(h, hipGetLastError());
    return GCSADMM_OK;
}

static bool state_ok(gcsadmm_handle h, const gcsadmm_state *st)
{
    if (!h || !st || !st->copy || !st->mu || !st->zedge || !st->xv || !st->zv || !st->yv) { if (h) h->err = "null state pointer"; return false; }
    if (!h->params_set) { h->err = "gcsadmm_reset has not been called"; return false; }
    return true;
}

static VertexLaunchDesc make_launch_desc(gcsadmm_handle h, const gcsadmm_state *st)
{
    VertexLaunchDesc d;
    d.step = make_step(h, st);
    d.n_waves = h->n_waves; d.n_special = h->n_special; d.all_m4 = h->all_m4; d.lds_bytes = h->lds_bytes; d.align_rows = h->align_rows;
    d.store_dl = h->store_dl; d.MM = h->MM;
    d.wave_slot_ptr = h->d_wave_slot_ptr; d.wave_vtx = h->d_wave_vtx; d.special_vtx = h->d_special_vtx; d.special_kind = h->d_special_kind;
    d.wave_order = h->d_wave_order; d.wave_iters = h->d_wave_iters;
    return d;
}

// ---- halo of a vertex partition: host-side helpers (C++ linkage) ----
// the checks of the halo lists, on the host alone: no allocation, no collective (gcsadmm_check_halo, and the head of attach_comm)
static gcsadmm_status halo_validate(gcsadmm_handle h, int rank, int world, const gcsadmm_halo_desc *hd)
{
    if (!hd || world < 1 || rank < 0 || rank >= world) { h->err = "bad communicator arguments"; return GCSADMM_ERR_BAD_ARG; }
    const int P = hd->num_peers;
    if (P < 0 || (P > 0 && (!hd->peer_rank || !hd->send_ptr || !hd->recv_ptr || !hd->send_cols || !hd->recv_cols))) { h->err = "null halo array"; return GCSADMM_ERR_BAD_ARG; }
    const int n_send = P ? hd->send_ptr[P] : 0, n_recv = P ? hd->recv_ptr[P] : 0;
    if (n_send != n_recv) { h->err = "halo lists: a partition sends and receives one column per cut edge and neighbour"; return GCSADMM_ERR_BAD_ARG; }
    for (int p = 0; p < P; ++p) {
        const int lo = hd->send_ptr[p], cnt = hd->send_ptr[p + 1] - lo;
        if (cnt < 0 || hd->recv_ptr[p + 1] - hd->recv_ptr[p] != cnt || hd->recv_ptr[p] != lo) { h->err = "halo lists: send and receive counts per peer must agree"; return GCSADMM_ERR_BAD_ARG; }
        if (hd->peer_rank[p] < 0 || hd->peer_rank[p] >= world || hd->peer_rank[p] == rank) { h->err = "halo lists: bad peer rank"; return GCSADMM_ERR_BAD_ARG; }
    }
    for (int j = 0; j < n_send; ++j) {
        if (hd->send_cols[j] < 0 || hd->send_cols[j] >= h->NI || hd->recv_cols[j] < 0 || hd->recv_cols[j] >= h->NI) { h->err = "halo lists: column out of range"; return GCSADMM_ERR_BAD_ARG; }
        if (!h->col_owned[hd->send_cols[j]]) { h->err = "halo lists: send column is not an owned incidence"; return GCSADMM_ERR_BAD_ARG; }
        if (h->col_owned[hd->recv_cols[j]]) { h->err = "halo lists: receive column is not a ghost column"; return GCSADMM_ERR_BAD_ARG; }
    }
    return GCSADMM_OK;
}

static void overlap_free(gcsadmm_handle h)
{
    for (void **p : {(void **)&h->d_split_ids, (void **)&h->d_split_order})
        if (*p) { (void)hipFree(*p); *p = nullptr; }
    if (h->ev_boundary) { (void)hipEventDestroy(h->ev_boundary); h->ev_boundary = nullptr; }
    if (h->ev_halo) { (void)hipEventDestroy(h->ev_halo); h->ev_halo = nullptr; }
    if (h->comm_stream) { (void)hipStreamDestroy(h->comm_stream); h->comm_stream = nullptr; }
    h->n_wave_b = 0;
}

// The split of the wavefronts for the overlapped loop: boundary = holds a vertex one of whose columns is sent to a neighbour.  Only for
// handles whose generic vertices all run the wavefront program (config 4's strips); mode 1 (tests) splits even without neighbours --
// the first quarter of the wavefronts plays the boundary -- so that the two launches, the second stream and the events can be
// exercised on one GPU.  Leaves n_wave_b = 0 when there is nothing to split.
static gcsadmm_status overlap_setup(gcsadmm_handle h, const gcsadmm_halo_desc *hd)
{
    overlap_free(h);
    if (h->overlap_mode == 2 || h->n_waves < 2 || h->n_wg > 0 || h->n_split > 0) return GCSADMM_OK;
    const int n_send = (hd && hd->num_peers > 0) ? hd->send_ptr[hd->num_peers] : 0;
    if (n_send == 0 && h->overlap_mode != 1) return GCSADMM_OK;
    std::vector<char> vb((size_t)std::max(h->V, 1), 0);
    for (int j = 0; j < n_send; ++j) {
        const int v = h->col_vertex[hd->send_cols[j]];
        if (v >= 0) vb[v] = 1;
    }
    std::vector<int> ids_b, ids_i;
    for (int w = 0; w < h->n_waves; ++w) {
        bool b = (n_send == 0) && w < std::max(1, h->n_waves / 4);
        for (int q = h->h_wave_slot_ptr[w]; q < h->h_wave_slot_ptr[w + 1] && !b; ++q) b = vb[h->h_wave_vtx[q]] != 0;
        (b ? ids_b : ids_i).push_back(w);
    }
    if (ids_b.empty() || ids_i.empty()) return GCSADMM_OK;      // nothing to overlap with
    h->n_wave_b = (int)ids_b.size();
    ids_b.insert(ids_b.end(), ids_i.begin(), ids_i.end());
    HIPCHK(h, upload(&h->d_split_ids, ids_b.data(), ids_b.size()));
    HIPCHK(h, upload(&h->d_split_order, ids_b.data(), ids_b.size()));
    if (!h->d_wave_iters) HIPCHK(h, upload(&h->d_wave_iters, (const int *)nullptr, (size_t)h->n_waves));
    HIPCHK(h, hipStreamCreateWithFlags(&h->comm_stream, hipStreamNonBlocking));
    HIPCHK(h, hipEventCreateWithFlags(&h->ev_boundary, hipEventDisableTiming));
    HIPCHK(h, hipEventCreateWithFlags(&h->ev_halo, hipEventDisableTiming));
    return GCSADMM_OK;
}

static void halo_free(gcsadmm_handle h)
{
    for (void **p : {(void **)&h->d_send_cols, (void **)&h->d_send_base, (void **)&h->d_send_stride, (void **)&h->d_recv_cols, (void **)&h->d_recv_base,
                     (void **)&h->d_recv_stride, &h->d_sendbuf, &h->d_recvbuf, (void **)&h->d_sums6})
        if (*p) { (void)hipFree(*p); *p = nullptr; }
    h->peers.clear(); h->peer_cnt.clear(); h->peer_off.clear(); h->n_send = h->n_recv = 0;
}

static gcsadmm_status halo_upload(gcsadmm_handle h, const gcsadmm_halo_desc *hd)
{
    const int P = hd->num_peers, c = h->c;
    h->peers.assign(hd->peer_rank, hd->peer_rank + P);
    h->peer_cnt.resize(P); h->peer_off.resize(P);
    h->n_send = P ? hd->send_ptr[P] : 0; h->n_recv = P ? hd->recv_ptr[P] : 0;
    std::vector<int> sbase(std::max(h->n_send, 1)), sstride(std::max(h->n_send, 1));
    for (int p = 0; p < P; ++p) {
        const int lo = hd->send_ptr[p], cnt = hd->send_ptr[p + 1] - lo;
        h->peer_cnt[p] = cnt; h->peer_off[p] = lo;
        for (int j = 0; j < cnt; ++j) { sbase[lo + j] = lo * c + j; sstride[lo + j] = cnt; }     // block of peer p: [c][cnt] at lo * c
    }
    const size_t esz = h->dtype == GCSADMM_F64 ? 8 : 4;
    HIPCHK(h, upload(&h->d_send_cols, hd->send_cols, (size_t)h->n_send));
    HIPCHK(h, upload(&h->d_recv_cols, hd->recv_cols, (size_t)h->n_recv));
    HIPCHK(h, upload(&h->d_send_base, sbase.data(), (size_t)h->n_send));
    HIPCHK(h, upload(&h->d_send_stride, sstride.data(), (size_t)h->n_send));
    HIPCHK(h, upload(&h->d_recv_base, sbase.data(), (size_t)h->n_recv));        // same block layout on the receiving side
    HIPCHK(h, upload(&h->d_recv_stride, sstride.data(), (size_t)h->n_recv));
    HIPCHK(h, hipMalloc(&h->d_sendbuf, std::max<size_t>((size_t)h->n_send * c * esz, 16)));
    HIPCHK(h, hipMalloc(&h->d_recvbuf, std::max<size_t>((size_t)h->n_recv * c * esz, 16)));
    // [0..6): this partition's five norms + inner failures, written by the edge step; [6..12): their sum over the ranks.  (Out of
    // place: after the stop test has fired the edge step no longer writes, and an in-place all-reduce would multiply the stale
    // values by `world` with every further iteration that was enqueued.)
    HIPCHK(h, upload(&h->d_sums6, (const double *)nullptr, 12));
    return GCSADMM_OK;
}

template <class T> static gcsadmm_status halo_pack(gcsadmm_handle h, const gcsadmm_state *st, hipStream_t s)
{
    if (h->n_send == 0) return GCSADMM_OK;
    const int tot = h->c * h->n_send;
    hipLaunchKernelGGL((halo_pack_kernel<T>), dim3((tot + 255) / 256), dim3(256), 0, s, h->c, h->n_send, h->NI, h->d_send_cols,
                       h->d_send_base, h->d_send_stride, (const T *)st->copy, (T *)h->d_sendbuf, h->d_cb);
    HIPCHK(h, hipGetLastError());
    return GCSADMM_OK;
}
template <class T> static gcsadmm_status halo_unpack(gcsadmm_handle h, const gcsadmm_state *st, hipStream_t s)
{
    if (h->n_recv == 0) return GCSADMM_OK;
    const int tot = h->c * h->n_recv;
    hipLaunchKernelGGL((halo_unpack_kernel<T>), dim3((tot + 255) / 256), dim3(256), 0, s, h->c, h->n_recv, h->NI, h->d_recv_cols,
                       h->d_recv_base, h->d_recv_stride, (const T *)h->d_recvbuf, (T *)st->copy, h->d_cb);
    HIPCHK(h, hipGetLastError());
    return GCSADMM_OK;
}

// the grouped point-to-point exchange of the packed halo (one message per neighbour and direction)
static gcsadmm_status halo_transfer(gcsadmm_handle h, hipStream_t s)
{
    if (h->peers.empty()) return GCSADMM_OK;
    if (!h->comm) { h->err = "halo exchange needs a communicator (gcsadmm_attach_comm with an id)"; return GCSADMM_ERR_BAD_ARG; }
    const ncclDataType_t dt = h->dtype == GCSADMM_F64 ? ncclFloat64 : ncclFloat32;
    const size_t esz = h->dtype == GCSADMM_F64 ? 8 : 4;
    NCCLCHK(h, rccl().GroupStart());
    for (size_t p = 0; p < h->peers.size(); ++p) {
        const size_t off = (size_t)h->peer_off[p] * h->c * esz, cnt = (size_t)h->peer_cnt[p] * h->c;
        NCCLCHK(h, rccl().Send((const char *)h->d_sendbuf + off, cnt, dt, h->peers[p], (ncclComm_t)h->comm, s));
        NCCLCHK(h, rccl().Recv((char *)h->d_recvbuf + off, cnt, dt, h->peers[p], (ncclComm_t)h->comm, s));
    }
    NCCLCHK(h, rccl().GroupEnd());
    return GCSADMM_OK;
}

extern "C" {

const char *gcsadmm_last_error(gcsadmm_handle h) { return h ? h->err.c_str() : g_create_error.c_str(); }

void gcsadmm_destroy(gcsadmm_handle h)
{
    if (!h) return;
    DeviceGuard device_guard_(h->device);
    void *ptrs[] = {h->d_inc_ptr, h->d_deg_in, h->d_inc_edge, h->d_poly_ptr, h->d_edge_inc_tail, h->d_edge_inc_head,
                    h->d_wave_slot_ptr, h->d_wave_vtx, h->d_special_vtx, h->d_special_kind, h->d_wg_vtx, h->d_poly_A, h->d_poly_bc,
                    h->d_center, h->d_inc_counted, h->d_edge_counted, h->d_cb, h->d_counters, h->d_partials, h->d_sums, h->d_ticket, h->d_prox_vtx, h->d_prox_counters,
                    h->d_warm, h->d_warm_ptr, h->d_wave_iters, h->d_wave_order, h->d_wg_iters, h->d_wg_order, h->d_split_vtx,
                    h->d_split_off, h->d_split_ws};
    for (void *p : ptrs)
        if (p) (void)hipFree(p);
    halo_free(h);
    overlap_free(h);
    if (h->d_term_ws) (void)hipFree(h->d_term_ws);
    if (h->d_term_rec) (void)hipFree(h->d_term_rec);
    if (h->ev_term_fork) (void)hipEventDestroy(h->ev_term_fork);
    if (h->ev_term_join) (void)hipEventDestroy(h->ev_term_join);
    if (h->term_stream) (void)hipStreamDestroy(h->term_stream);
    if (h->comm && rccl().ok()) (void)rccl().CommDestroy((ncclComm_t)h->comm);
    for (auto ev : h->events) (void)hipEventDestroy(ev);
    delete h;
}

gcsadmm_status gcsadmm_create(const gcsadmm_graph_desc *g, gcsadmm_handle *out)
{
    if (out) *out = nullptr;
    auto fail = [&](gcsadmm_status st, const std::string &msg) { g_create_error = msg; return st; };
    std::string msg;
    gcsadmm_status st;
    if (!out) return fail(GCSADMM_ERR_BAD_ARG, "null descriptor or output pointer");
    if ((st = check_graph_desc(g, msg)) != GCSADMM_OK) return fail(st, msg);
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) return fail(GCSADMM_ERR_NO_DEVICE, "no HIP device");
    if (g->device < 0 || g->device >= ndev) return fail(GCSADMM_ERR_BAD_ARG, "device ordinal out of range");
    CreatePlan p;
    if ((st = make_create_plan(*g, p, msg)) != GCSADMM_OK) return fail(st, msg);

    const int V = g->num_vertices, E = g->num_edges, n = g->n, NIo = g->inc_ptr[V], MT = g->poly_ptr[V];
    auto *h = new (std::nothrow) gcsadmm_handle_s;
    if (!h) return fail(GCSADMM_ERR_HIP, "out of host memory");
    h->n = n; h->V = V; h->E = E; h->NI = g->num_incidences; h->NI_owned = NIo; h->c = 2 * n + 1; h->MM = p.wave_mm;
    h->edge_major = g->edge_major_columns;
    h->col_owned = std::move(p.col_owned); h->col_vertex = std::move(p.col_vertex);
    h->h_wave_slot_ptr = p.wave_slot_ptr; h->h_wave_vtx = p.wave_vtx;
    h->dtype = g->state_dtype; h->device = g->device;
    h->n_waves = p.n_waves(); h->n_special = (int)p.special_vtx.size();
    h->slots_cap = p.slots_cap; h->all_m4 = p.all_m4; h->align_rows = p.align_rows; h->store_dl = p.store_dl; h->lds_bytes = p.lds_bytes;
    h->n_wg = (int)p.wg_vtx.size(); h->wg_lds_bytes = p.wg_lds_bytes; h->wg_box = p.wg_box; h->wg_t512 = p.wg_t512;
    h->n_split = (int)p.split_vtx.size(); h->split_lds_bytes = p.split_lds_bytes; h->split_doubles = (size_t)p.split_doubles;
    h->nx = p.nx; h->nmu = p.nmu;
    h->edge_unroll = p.edge_unroll; h->edge_blocks = p.edge_blocks;
    auto bail = [&](hipError_t e, const char *what) {
        g_create_error = std::string(what) + ": " + hipGetErrorString(e);
        gcsadmm_destroy(h);
        return GCSADMM_ERR_HIP;
    };
    hipError_t e;
    DeviceGuard device_guard_(g->device);
    if ((e = device_guard_.err) != hipSuccess) return bail(e, "hipSetDevice");
#define UP(dst, src, cnt) if ((e = upload(&h->dst, src, (size_t)(cnt))) != hipSuccess) return bail(e, "upload " #dst)
    UP(d_inc_ptr, g->inc_ptr, V + 1);
    UP(d_deg_in, p.deg_in.data(), V);
    UP(d_inc_edge, g->inc_edge, NIo);
    UP(d_poly_ptr, g->poly_ptr, V + 1);
    UP(d_edge_inc_tail, g->edge_inc_tail, E);
    UP(d_edge_inc_head, g->edge_inc_head, E);
    UP(d_wave_slot_ptr, p.wave_slot_ptr.data(), p.wave_slot_ptr.size());
    UP(d_wave_vtx, p.wave_vtx.data(), p.wave_vtx.size());
    UP(d_special_vtx, p.special_vtx.data(), p.special_vtx.size());
    UP(d_special_kind, p.special_kind.data(), p.special_kind.size());
    UP(d_wg_vtx, p.wg_vtx.data(), p.wg_vtx.size());
    if (h->n_split > 0) {
        UP(d_split_vtx, p.split_vtx.data(), p.split_vtx.size());
        UP(d_split_off, p.split_off.data(), p.split_off.size());
        UP(d_split_ws, (const double *)nullptr, h->split_doubles);
    }
    UP(d_poly_A, g->poly_A, (size_t)MT * n);
    UP(d_poly_bc, p.bc.data(), MT);
    UP(d_center, g->center, (size_t)V * n);
    if (g->inc_counted) UP(d_inc_counted, g->inc_counted, g->num_incidences);
    if (g->edge_counted) UP(d_edge_counted, g->edge_counted, E);
    UP(d_cb, (const gcsadmm_control_block *)nullptr, 1);
    UP(d_counters, (const int *)nullptr, 2);
    UP(d_partials, (const double *)nullptr, (size_t)h->edge_blocks * 5);
    UP(d_sums, (const double *)nullptr, 5);
    UP(d_ticket, (const unsigned *)nullptr, 1);
    if (p.n_term > 0) {       // region terminals: workspace, an auxiliary stream and the fork / join events
        h->n_term = p.n_term;
        for (int i = 0; i < p.n_term; ++i) {
            h->term_vtx[i] = p.term_vtx[i]; h->term_is_src[i] = p.term_is_src[i];
            h->term_ws_off[i] = p.term_ws_off[i]; h->term_rec_off[i] = p.term_rec_off[i];
        }
        h->term_lds_doubles = p.term_lds_doubles; h->term_threads = p.term_threads;
        UP(d_term_ws, (const double *)nullptr, (size_t)p.term_ws_doubles);
        h->term_rec_doubles = (size_t)p.term_rec_doubles;
        UP(d_term_rec, (const double *)nullptr, h->term_rec_doubles);
        if ((e = hipStreamCreateWithFlags(&h->term_stream, hipStreamNonBlocking)) != hipSuccess) return bail(e, "hipStreamCreate");
        if ((e = hipEventCreateWithFlags(&h->ev_term_fork, hipEventDisableTiming)) != hipSuccess) return bail(e, "hipEventCreate");
        if ((e = hipEventCreateWithFlags(&h->ev_term_join, hipEventDisableTiming)) != hipSuccess) return bail(e, "hipEventCreate");
    }
    h->warm_doubles = (size_t)p.warm_ptr[V];
    UP(d_warm_ptr, p.warm_ptr.data(), V + 1);
    UP(d_warm, (const double *)nullptr, h->warm_doubles);
    {   // slowest-first dispatch: only where a launch needs more than one round of the chip (small graphs run all at once)
        std::vector<int> iota(std::max(std::max(h->n_waves, h->n_wg), 1));
        for (size_t i = 0; i < iota.size(); ++i) iota[i] = (int)i;
        if (p.wave_reorder) { UP(d_wave_iters, (const int *)nullptr, h->n_waves); UP(d_wave_order, iota.data(), h->n_waves); }
        if (p.wg_reorder) { UP(d_wg_iters, (const int *)nullptr, h->n_wg); UP(d_wg_order, iota.data(), h->n_wg); }
    }
    h->n_prox = (int)p.prox_vtx.size(); h->src = g->src; h->dst = g->dst; h->prox_lds_bytes = p.prox_lds_bytes;
    UP(d_prox_vtx, p.prox_vtx.data(), p.prox_vtx.size());
    UP(d_prox_counters, (const int *)nullptr, 2);
#undef UP
    if (h->lds_bytes > 48 * 1024) {
        e = h->dtype == GCSADMM_F64 ? set_lds_attr<2, double>(h->all_m4, h->lds_bytes) : set_lds_attr<2, float>(h->all_m4, h->lds_bytes);
        if (e != hipSuccess) return bail(e, "hipFuncSetAttribute(MaxDynamicSharedMemorySize)");
    }
    if (h->wg_lds_bytes > 48 * 1024 && (e = h->wg_t512 ? gcsadmm_wg_set_lds_t512(h->n, h->dtype, h->wg_lds_bytes)
                                                        : gcsadmm_wg_set_lds(h->n, h->dtype, h->wg_lds_bytes)) != hipSuccess)
        return bail(e, "hipFuncSetAttribute(MaxDynamicSharedMemorySize, workgroup program)");
    if (h->split_lds_bytes > 48 * 1024 && (e = gcsadmm_wg_set_split_lds(h->n, h->dtype, h->split_lds_bytes)) != hipSuccess)
        return bail(e, "hipFuncSetAttribute(MaxDynamicSharedMemorySize, split workgroup program)");
    *out = h;
    return GCSADMM_OK;
}

gcsadmm_status gcsadmm_reset(gcsadmm_handle h, const gcsadmm_params *p, void *stream)
{
    if (!h || !p) return GCSADMM_ERR_BAD_ARG;
    if (!(p->rho > 0) || p->max_it < 1 || !(p->ipm_tol > 0) || p->ipm_max_iter < 1) { h->err = "bad parameter"; return GCSADMM_ERR_BAD_ARG; }
    h->params = *p; h->params_set = true;
    gcsadmm_control_block cb{};
    cb.rho = p->rho; cb.mu_scale = 1.0; cb.it = 1; cb.status = GCSADMM_RUNNING;
    USE_DEVICE(h);
    HIPCHK(h, hipMemcpyAsync(h->d_cb, &cb, sizeof(cb), hipMemcpyHostToDevice, (hipStream_t)stream));
    HIPCHK(h, hipMemsetAsync(h->d_counters, 0, 2 * sizeof(int), (hipStream_t)stream));
    // a new run starts without warm-start records (runs from the same state are then identical, whatever ran before)
    if (h->warm_doubles > 0) HIPCHK(h, hipMemsetAsync(h->d_warm, 0, h->warm_doubles * sizeof(double), (hipStream_t)stream));
    if (h->term_rec_doubles > 0) HIPCHK(h, hipMemsetAsync(h->d_term_rec, 0, h->term_rec_doubles * sizeof(double), (hipStream_t)stream));
    h->vertex_steps = 0;
    if (h->d_split_order) HIPCHK(h, hipMemcpyAsync(h->d_split_order, h->d_split_ids, sizeof(int) * (size_t)h->n_waves, hipMemcpyDeviceToDevice, (hipStream_t)stream));
    for (auto po : {std::make_pair(h->d_wave_order, h->n_waves), std::make_pair(h->d_wg_order, h->n_wg)})
        if (po.first) {
            std::vector<int> iota(po.second);
            for (int i = 0; i < po.second; ++i) iota[i] = i;
            HIPCHK(h, hipMemcpyAsync(po.first, iota.data(), sizeof(int) * po.second, hipMemcpyHostToDevice, (hipStream_t)stream));
            HIPCHK(h, hipStreamSynchronize((hipStream_t)stream));      // iota is a stack object
        }
    HIPCHK(h, hipStreamSynchronize((hipStream_t)stream));   // cb is a stack object
    return GCSADMM_OK;
}

gcsadmm_status gcsadmm_vertex_step(gcsadmm_handle h, const gcsadmm_state *st, void *stream)
{
    if (!state_ok(h, st)) return GCSADMM_ERR_BAD_ARG;
    USE_DEVICE(h);
    return h->dtype == GCSADMM_F64 ? launch_vertex<double>(h, st, (hipStream_t)stream) : launch_vertex<float>(h, st, (hipStream_t)stream);
}

gcsadmm_status gcsadmm_edge_step(gcsadmm_handle h, const gcsadmm_state *st, double *sums_dev, void *stream)
{
    if (!state_ok(h, st) || !sums_dev) return GCSADMM_ERR_BAD_ARG;
    USE_DEVICE(h);
    return h->dtype == GCSADMM_F64 ? launch_edge<double>(h, st, sums_dev, (hipStream_t)stream) : launch_edge<float>(h, st, sums_dev, (hipStream_t)stream);
}

gcsadmm_status gcsadmm_control(gcsadmm_handle h, const double *sums_dev, double *trace_dev, void *stream)
{
    if (!h || !sums_dev || !h->params_set) return GCSADMM_ERR_BAD_ARG;
    USE_DEVICE(h);
    const gcsadmm_params &p = h->params;
    ControlParams cp{p.tau_incr, p.tau_decr, p.nu, p.eps_abs, p.eps_rel, h->nx, h->nmu, p.it_rho_limit, p.max_it};
    hipLaunchKernelGGL(control_kernel, dim3(1), dim3(1), 0, (hipStream_t)stream, h->d_cb, sums_dev, cp, h->d_counters, trace_dev, false);
    HIPCHK(h, hipGetLastError());
    return GCSADMM_OK;
}

gcsadmm_status gcsadmm_run(gcsadmm_handle h, const gcsadmm_state *st, int32_t k, double *trace_dev, void *stream)
{
    if (!state_ok(h, st) || k < 0) return GCSADMM_ERR_BAD_ARG;
    USE_DEVICE(h);      // (the edge launches below are issued from here, not through an entry point that guards for itself)
    for (int i = 0; i < k; ++i) {
        gcsadmm_status s;
        if ((s = gcsadmm_vertex_step(h, st, stream)) != GCSADMM_OK) return s;
        // edge step and control step in two launches (one when all edges fit a single workgroup)
        s = h->dtype == GCSADMM_F64 ? launch_edge<double>(h, st, h->d_sums, (hipStream_t)stream, true, trace_dev)
                                    : launch_edge<float>(h, st, h->d_sums, (hipStream_t)stream, true, trace_dev);
        if (s != GCSADMM_OK) return s;
    }
    return GCSADMM_OK;
}

// =================================================================================================
// vertex partitions across GPUs: one handle per rank, RCCL over xGMI.
// Per iteration, all on one stream with no host synchronisation:
//   vertex step -> pack the cut edges' copies per neighbour -> grouped ncclSend / ncclRecv -> unpack into the ghost columns
//   -> edge step on local + ghost columns -> ncclAllReduce(sum) of the five norms and the inner-failure count (6 doubles)
//   -> control (every rank takes the same decision from the same numbers).
// Both messages are latency-bound at every configuration of BASELINE.json (about 25 KB per boundary of the 100k lattice,
// 48 bytes for the all-reduce).
// =================================================================================================
gcsadmm_status gcsadmm_comm_unique_id(void *id128)
{
    if (!id128) return GCSADMM_ERR_BAD_ARG;
    if (!rccl().ok()) { g_create_error = rccl().err; return GCSADMM_ERR_HIP; }
    static_assert(sizeof(ncclUniqueId) == 128, "ncclUniqueId is 128 bytes");
    ncclUniqueId id;
    if (rccl().GetUniqueId(&id) != ncclSuccess) { g_create_error = "ncclGetUniqueId failed"; return GCSADMM_ERR_HIP; }
    std::memcpy(id128, &id, sizeof(id));
    return GCSADMM_OK;
}

gcsadmm_status gcsadmm_check_halo(gcsadmm_handle h, int32_t rank, int32_t world, const gcsadmm_halo_desc *halo)
{
    if (!h) return GCSADMM_ERR_BAD_ARG;
    if (h->d_sums6) { h->err = "a communicator is already attached"; return GCSADMM_ERR_BAD_ARG; }
    return halo_validate(h, rank, world, halo);
}

gcsadmm_status gcsadmm_attach_comm(gcsadmm_handle h, int32_t rank, int32_t world, const void *id128, const gcsadmm_halo_desc *halo)
{
    // everything that can fail on this rank alone comes first: a rank must not return an error while its peers wait in the collective
    gcsadmm_status st = gcsadmm_check_halo(h, rank, world, halo);
    if (st != GCSADMM_OK) return st;
    if (id128 && !rccl().ok()) { h->err = rccl().err; return GCSADMM_ERR_HIP; }
    USE_DEVICE(h);
    h->rank = rank; h->world = world;
    if ((st = halo_upload(h, halo)) != GCSADMM_OK) { halo_free(h); return st; }
    if (id128) {      // id128 == NULL: no communicator (the host moves the packed buffers itself; gcsadmm_run_partitioned needs one)
        ncclUniqueId id;
        std::memcpy(&id, id128, sizeof(id));
        ncclComm_t comm = nullptr;
        const ncclResult_t r = rccl().CommInitRank(&comm, world, id, rank);
        if (r != ncclSuccess) {      // not attached: the handle can be attached again
            h->err = std::string("ncclCommInitRank: ") + (rccl().GetErrorString ? rccl().GetErrorString(r) : "RCCL error");
            halo_free(h);
            return GCSADMM_ERR_HIP;
        }
        h->comm = comm;
    }
    return overlap_setup(h, halo);
}

gcsadmm_status gcsadmm_halo_pack(gcsadmm_handle h, const gcsadmm_state *st, void *stream)
{
    if (!state_ok(h, st) || !h->d_sums6) { if (h) h->err = "no halo attached"; return GCSADMM_ERR_BAD_ARG; }
    USE_DEVICE(h);
    return h->dtype == GCSADMM_F64 ? halo_pack<double>(h, st, (hipStream_t)stream) : halo_pack<float>(h, st, (hipStream_t)stream);
}
gcsadmm_status gcsadmm_halo_unpack(gcsadmm_handle h, const gcsadmm_state *st, void *stream)
{
    if (!state_ok(h, st) || !h->d_sums6) { if (h) h->err = "no halo attached"; return GCSADMM_ERR_BAD_ARG; }
    USE_DEVICE(h);
    return h->dtype == GCSADMM_F64 ? halo_unpack<double>(h, st, (hipStream_t)stream) : halo_unpack<float>(h, st, (hipStream_t)stream);
}
gcsadmm_status gcsadmm_halo_buffers(gcsadmm_handle h, void **send_buf, void **recv_buf, int64_t *num_elements)
{
    if (!h || !h->d_sums6) { if (h) h->err = "no halo attached"; return GCSADMM_ERR_BAD_ARG; }
    if (send_buf) *send_buf = h->d_sendbuf;
    if (recv_buf) *recv_buf = h->d_recvbuf;
    if (num_elements) *num_elements = (int64_t)h->c * h->n_send;
    return GCSADMM_OK;
}

gcsadmm_status gcsadmm_halo_exchange(gcsadmm_handle h, const gcsadmm_state *st, void *stream)
{
    if (!state_ok(h, st) || !h->d_sums6) { if (h) h->err = "no halo attached"; return GCSADMM_ERR_BAD_ARG; }
    USE_DEVICE(h);
    hipStream_t s = (hipStream_t)stream;
    gcsadmm_status r;
    if ((r = h->dtype == GCSADMM_F64 ? halo_pack<double>(h, st, s) : halo_pack<float>(h, st, s)) != GCSADMM_OK) return r;
    if ((r = halo_transfer(h, s)) != GCSADMM_OK) return r;
    return h->dtype == GCSADMM_F64 ? halo_unpack<double>(h, st, s) : halo_unpack<float>(h, st, s);
}

// one loop for gcsadmm_run_partitioned and its event-bracketed twin: ev != nullptr records 6 events per iteration on the stream
// (before / after the vertex step, after the halo exchange, after the edge step, after the all-reduce, after the control step)
static gcsadmm_status run_partitioned_loop(gcsadmm_handle h, const gcsadmm_state *st, int k, double *trace_dev, hipStream_t s, hipEvent_t *ev)
{
    const gcsadmm_params &pp = h->params;
    const ControlParams cp{pp.tau_incr, pp.tau_decr, pp.nu, pp.eps_abs, pp.eps_rel, h->nx, h->nmu, pp.it_rho_limit, pp.max_it};
    if (!h->comm && h->world > 1) { h->err = "gcsadmm_run_partitioned needs a communicator (gcsadmm_attach_comm with an id)"; return GCSADMM_ERR_BAD_ARG; }
    // OVERLAPPED form (not for the stage-timed twin, whose events want one stream): the wavefronts that hold a vertex with a
    // cut edge are launched FIRST and on a second stream, with pack, grouped send / recv and unpack of the halo behind them; the interior
    // wavefronts are launched on the caller's stream at the same time, and the edge step waits for both.  Same kernels, same numbers: the
    // split only changes what runs when.
    //   s : [ev_boundary = previous iteration done] -> interior launch -> wait [ev_halo] -> edge step -> all-reduce -> control
    //   sc: wait [ev_boundary] -> boundary launch (+ closed-form vertices) -> pack -> send / recv -> unpack -> [ev_halo]
    // (The two launches must be CONCURRENT: one after the other on one stream each waits for its own slowest wavefront -- measured on a
    // strip of 12.6 k vertices, 348 -> 509 us per iteration.  RCCL orders the operations of one communicator across streams itself;
    // every rank issues them in the same order.)
    const bool overlap = !ev && h->n_wave_b > 0 && h->overlap_mode != 2;
    for (int i = 0; i < k && overlap; ++i) {
        gcsadmm_status r;
        const bool f64 = h->dtype == GCSADMM_F64;
        const bool reorder = ++h->vertex_steps % REORDER_EVERY == 0;
        HIPCHK(h, hipEventRecord(h->ev_boundary, s));
        HIPCHK(h, hipStreamWaitEvent(h->comm_stream, h->ev_boundary, 0));
        if ((r = f64 ? launch_vertex<double>(h, st, h->comm_stream, 0, reorder) : launch_vertex<float>(h, st, h->comm_stream, 0, reorder)) != GCSADMM_OK) return r;
        if ((r = gcsadmm_halo_exchange(h, st, (void *)h->comm_stream)) != GCSADMM_OK) return r;
        HIPCHK(h, hipEventRecord(h->ev_halo, h->comm_stream));
        if ((r = f64 ? launch_vertex<double>(h, st, s, 1, reorder) : launch_vertex<float>(h, st, s, 1, reorder)) != GCSADMM_OK) return r;
        HIPCHK(h, hipStreamWaitEvent(s, h->ev_halo, 0));
        r = f64 ? launch_edge<double>(h, st, h->d_sums6, s, false, nullptr, true) : launch_edge<float>(h, st, h->d_sums6, s, false, nullptr, true);
        if (r != GCSADMM_OK) return r;
        const double *reduced = h->d_sums6;
        if (h->comm) {
            NCCLCHK(h, rccl().AllReduce(h->d_sums6, h->d_sums6 + 6, 6, ncclFloat64, ncclSum, (ncclComm_t)h->comm, s));
            reduced = h->d_sums6 + 6;
        }
        hipLaunchKernelGGL(control_kernel, dim3(1), dim3(1), 0, s, h->d_cb, reduced, cp, h->d_counters, trace_dev, true);
        HIPCHK(h, hipGetLastError());
    }
    if (overlap) {      // the caller's stream is the one the caller synchronises: nothing of this call may still run on the other
        HIPCHK(h, hipEventRecord(h->ev_halo, h->comm_stream));
        HIPCHK(h, hipStreamWaitEvent(s, h->ev_halo, 0));
        return GCSADMM_OK;
    }
    for (int i = 0; i < k; ++i) {
        gcsadmm_status r;
        if (ev) HIPCHK(h, hipEventRecord(ev[6 * i + 0], s));
        if ((r = gcsadmm_vertex_step(h, st, (void *)s)) != GCSADMM_OK) return r;
        if (ev) HIPCHK(h, hipEventRecord(ev[6 * i + 1], s));
        if ((r = gcsadmm_halo_exchange(h, st, (void *)s)) != GCSADMM_OK) return r;
        if (ev) HIPCHK(h, hipEventRecord(ev[6 * i + 2], s));
        r = h->dtype == GCSADMM_F64 ? launch_edge<double>(h, st, h->d_sums6, s, false, nullptr, true)
                                    : launch_edge<float>(h, st, h->d_sums6, s, false, nullptr, true);      // sums + failure count, one launch
        if (r != GCSADMM_OK) return r;
        if (ev) HIPCHK(h, hipEventRecord(ev[6 * i + 3], s));
        const double *reduced = h->d_sums6;
        if (h->comm) {
            NCCLCHK(h, rccl().AllReduce(h->d_sums6, h->d_sums6 + 6, 6, ncclFloat64, ncclSum, (ncclComm_t)h->comm, s));
            reduced = h->d_sums6 + 6;
        }
        if (ev) HIPCHK(h, hipEventRecord(ev[6 * i + 4], s));
        hipLaunchKernelGGL(control_kernel, dim3(1), dim3(1), 0, s, h->d_cb, reduced, cp, h->d_counters, trace_dev, true);
        HIPCHK(h, hipGetLastError());
        if (ev) HIPCHK(h, hipEventRecord(ev[6 * i + 5], s));
    }
    return GCSADMM_OK;
}

gcsadmm_status gcsadmm_run_partitioned(gcsadmm_handle h, const gcsadmm_state *st, int32_t k, double *trace_dev, void *stream)
{
    if (!state_ok(h, st) || k < 0) return GCSADMM_ERR_BAD_ARG;
    if (!h->d_sums6) { h->err = "gcsadmm_attach_comm has not been called"; return GCSADMM_ERR_BAD_ARG; }
    USE_DEVICE(h);
    return run_partitioned_loop(h, st, k, trace_dev, (hipStream_t)stream, nullptr);
}

gcsadmm_status gcsadmm_run_partitioned_timed(gcsadmm_handle h, const gcsadmm_state *st, int32_t k, double *trace_dev, void *stream,
                                             float *vertex_ms, float *halo_ms, float *edge_ms, float *reduce_ms)
{
    if (!state_ok(h, st) || k < 0 || !vertex_ms || !halo_ms || !edge_ms || !reduce_ms) return GCSADMM_ERR_BAD_ARG;
    if (!h->d_sums6) { h->err = "gcsadmm_attach_comm has not been called"; return GCSADMM_ERR_BAD_ARG; }
    USE_DEVICE(h);
    hipStream_t s = (hipStream_t)stream;
    while (h->events.size() < (size_t)6 * k) {
        hipEvent_t e;
        HIPCHK(h, hipEventCreate(&e));
        h->events.push_back(e);
    }
    gcsadmm_status r = run_partitioned_loop(h, st, k, trace_dev, s, h->events.data());
    if (r != GCSADMM_OK) return r;
    HIPCHK(h, hipStreamSynchronize(s));
    double acc[4] = {0, 0, 0, 0};
    for (int i = 0; i < k; ++i) {
        float t = 0;
        HIPCHK(h, hipEventElapsedTime(&t, h->events[6 * i + 0], h->events[6 * i + 1])); acc[0] += t;
        HIPCHK(h, hipEventElapsedTime(&t, h->events[6 * i + 1], h->events[6 * i + 2])); acc[1] += t;
        HIPCHK(h, hipEventElapsedTime(&t, h->events[6 * i + 2], h->events[6 * i + 3])); acc[2] += t;
        HIPCHK(h, hipEventElapsedTime(&t, h->events[6 * i + 3], h->events[6 * i + 5])); acc[3] += t;
    }
    *vertex_ms = (float)acc[0]; *halo_ms = (float)acc[1]; *edge_ms = (float)acc[2]; *reduce_ms = (float)acc[3];
    return GCSADMM_OK;
}

gcsadmm_status gcsadmm_set_overlap(gcsadmm_handle h, int32_t mode, int32_t *boundary_units)
{
    if (!h || mode < 0 || mode > 2) return GCSADMM_ERR_BAD_ARG;
    if (boundary_units) *boundary_units = 0;
    if (!h->d_sums6) { h->err = "gcsadmm_attach_comm has not been called"; return GCSADMM_ERR_BAD_ARG; }
    USE_DEVICE(h);
    h->overlap_mode = mode;
    // the split is derived from the halo lists uploaded at attach: rebuild them as a descriptor of host arrays
    std::vector<int> send_cols((size_t)std::max(h->n_send, 1)), ptr(h->peers.size() + 1, 0);
    if (h->n_send > 0) HIPCHK(h, hipMemcpy(send_cols.data(), h->d_send_cols, sizeof(int) * (size_t)h->n_send, hipMemcpyDeviceToHost));
    for (size_t p = 0; p < h->peers.size(); ++p) ptr[p + 1] = ptr[p] + h->peer_cnt[p];
    gcsadmm_halo_desc hd{};
    hd.num_peers = (int)h->peers.size(); hd.peer_rank = h->peers.data(); hd.send_ptr = ptr.data(); hd.send_cols = send_cols.data();
    hd.recv_ptr = ptr.data(); hd.recv_cols = send_cols.data();
    const gcsadmm_status r = overlap_setup(h, &hd);
    if (boundary_units) *boundary_units = h->n_wave_b;
    return r;
}

gcsadmm_status gcsadmm_comm_count(gcsadmm_handle h, int32_t *count)
{
    if (!h || !count) return GCSADMM_ERR_BAD_ARG;
    *count = 0;
    if (!h->comm) return GCSADMM_OK;        // no communicator attached (single handle, or a host-side transport)
    if (!rccl().CommCount) { h->err = "librccl lacks ncclCommCount"; return GCSADMM_ERR_HIP; }
    USE_DEVICE(h);
    int n = 0;
    NCCLCHK(h, rccl().CommCount((ncclComm_t)h->comm, &n));
    *count = n;
    return GCSADMM_OK;
}

gcsadmm_status gcsadmm_vertex_prox(gcsadmm_handle h, const double *q_dev, const double *c_dev, double *xv_dev, double *zv_dev,
                                   double *yv_dev, double ipm_tol, int32_t ipm_max_iter, int32_t *failures_host, void *stream)
{
    if (!h || !q_dev || !c_dev || !xv_dev || !zv_dev || !yv_dev || !(ipm_tol > 0) || ipm_max_iter < 1) { if (h) h->err = "bad prox argument"; return GCSADMM_ERR_BAD_ARG; }
    if (h->prox_lds_bytes > 160 * 1024) { h->err = "facet count too large for LDS"; return GCSADMM_ERR_UNSUPPORTED; }
    if (h->n_term > 0) { h->err = "the prox kernel (v1 x-update) takes its terminals as points; this graph has a terminal that is a region"; return GCSADMM_ERR_UNSUPPORTED; }
    USE_DEVICE(h);
    hipStream_t s = (hipStream_t)stream;
    HIPCHK(h, hipMemsetAsync(h->d_prox_counters, 0, 2 * sizeof(int), s));
    WgLaunchDesc d{};
    d.n = h->n; d.dtype = GCSADMM_F64; d.n_vtx = h->n_prox; d.lds_bytes = h->prox_lds_bytes; d.vtx = h->d_prox_vtx;
    StepDesc &p = d.step;     // the ADMM state, the edge tolerance and the warm start stay unset: the PROX solve reads none of them
    p.inc_ptr = h->d_inc_ptr; p.deg_in = h->d_deg_in; p.inc_edge = h->d_inc_edge; p.poly_ptr = h->d_poly_ptr;
    p.poly_A = h->d_poly_A; p.poly_bc = h->d_poly_bc; p.center = h->d_center;
    p.xv = xv_dev; p.zv = zv_dev; p.yv = yv_dev; p.counters = h->d_prox_counters; p.ipm_tol = ipm_tol; p.ipm_max_iter = ipm_max_iter;
    gcsadmm_wg_launch_prox(d, q_dev, c_dev, h->src, h->dst, s);
    HIPCHK(h, hipGetLastError());
    if (failures_host) {      // optional: synchronises the stream
        int cnt[2] = {0, 0};
        HIPCHK(h, hipMemcpyAsync(cnt, h->d_prox_counters, sizeof(cnt), hipMemcpyDeviceToHost, s));
        HIPCHK(h, hipStreamSynchronize(s));
        *failures_host = cnt[0];
    }
    return GCSADMM_OK;
}

gcsadmm_status gcsadmm_run_timed(gcsadmm_handle h, const gcsadmm_state *st, int32_t k, double *trace_dev, void *stream,
                                 float *vertex_ms, int32_t *vertex_launches, float *edge_ms, int32_t *edge_launches)
{
    if (!state_ok(h, st) || k < 0 || !vertex_ms || !edge_ms || !vertex_launches || !edge_launches) return GCSADMM_ERR_BAD_ARG;
    USE_DEVICE(h);
    hipStream_t s = (hipStream_t)stream;
    const size_t need = (size_t)4 * k;
    while (h->events.size() < need) {
        hipEvent_t ev;
        HIPCHK(h, hipEventCreate(&ev));
        h->events.push_back(ev);
    }
    for (int i = 0; i < k; ++i) {
        gcsadmm_status r;
        HIPCHK(h, hipEventRecord(h->events[4 * i + 0], s));
        if ((r = gcsadmm_vertex_step(h, st, stream)) != GCSADMM_OK) return r;
        HIPCHK(h, hipEventRecord(h->events[4 * i + 1], s));
        HIPCHK(h, hipEventRecord(h->events[4 * i + 2], s));
        r = h->dtype == GCSADMM_F64 ? launch_edge<double>(h, st, h->d_sums, s, true, trace_dev) : launch_edge<float>(h, st, h->d_sums, s, true, trace_dev);
        if (r != GCSADMM_OK) return r;
        HIPCHK(h, hipEventRecord(h->events[4 * i + 3], s));
    }
    HIPCHK(h, hipStreamSynchronize(s));
    double vm = 0, em = 0;
    for (int i = 0; i < k; ++i) {
        float t = 0;
        HIPCHK(h, hipEventElapsedTime(&t, h->events[4 * i + 0], h->events[4 * i + 1])); vm += t;
        HIPCHK(h, hipEventElapsedTime(&t, h->events[4 * i + 2], h->events[4 * i + 3])); em += t;
    }
    *vertex_ms = (float)vm; *edge_ms = (float)em; *vertex_launches = k; *edge_launches = k;
    return GCSADMM_OK;
}

gcsadmm_status gcsadmm_read_control(gcsadmm_handle h, gcsadmm_control_block *out, void *stream)
{
    if (!h || !out) return GCSADMM_ERR_BAD_ARG;
    USE_DEVICE(h);
    HIPCHK(h, hipMemcpyAsync(out, h->d_cb, sizeof(*out), hipMemcpyDeviceToHost, (hipStream_t)stream));
    HIPCHK(h, hipStreamSynchronize((hipStream_t)stream));
    return GCSADMM_OK;
}

gcsadmm_status gcsadmm_cost(gcsadmm_handle h, const gcsadmm_state *st, double eps_edge, double *cost_dev, void *stream)
{
    if (!h || !st || !st->zv || !st->zedge || !cost_dev) return GCSADMM_ERR_BAD_ARG;
    USE_DEVICE(h);
    if (h->dtype == GCSADMM_F64)
        hipLaunchKernelGGL((cost_kernel<double>), dim3(1), dim3(256), 0, (hipStream_t)stream, h->V, h->E, h->n, st->zv,
                           (const double *)st->zedge, h->d_edge_counted, eps_edge, cost_dev);
    else
        hipLaunchKernelGGL((cost_kernel<float>), dim3(1), dim3(256), 0, (hipStream_t)stream, h->V, h->E, h->n, st->zv,
                           (const float *)st->zedge, h->d_edge_counted, eps_edge, cost_dev);
    HIPCHK(h, hipGetLastError());
    return GCSADMM_OK;
}

#ifdef GCS_PHASE_TIMING
int gcsadmm_debug_sub_cycles(unsigned long long *out16)
{
    return (int)hipMemcpyFromSymbol(out16, HIP_SYMBOL(g_sub_cycles), 16 * sizeof(unsigned long long));
}

int gcsadmm_debug_phase_cycles(unsigned long long *out64)
{
    return (int)hipMemcpyFromSymbol(out64, HIP_SYMBOL(g_phase_cycles), 64 * sizeof(unsigned long long));
}
#endif

gcsadmm_status gcsadmm_query(gcsadmm_handle h, int32_t *num_waves, int32_t *lds_bytes, int32_t *num_special,
                             int32_t *num_workgroup_vertices, int32_t *workgroup_lds_bytes)
{
    if (!h) return GCSADMM_ERR_BAD_ARG;
    if (num_waves) *num_waves = h->n_waves;
    if (lds_bytes) *lds_bytes = h->lds_bytes;
    if (num_special) *num_special = h->n_special;
    if (num_workgroup_vertices) *num_workgroup_vertices = h->n_wg;
    if (workgroup_lds_bytes) *workgroup_lds_bytes = h->wg_lds_bytes;
    return GCSADMM_OK;
}

gcsadmm_status gcsadmm_query_workspace(gcsadmm_handle h, int32_t *num_split_vertices, int32_t *split_lds_bytes, int64_t *workspace_bytes)
{
    if (!h) return GCSADMM_ERR_BAD_ARG;
    if (num_split_vertices) *num_split_vertices = h->n_split;
    if (split_lds_bytes) *split_lds_bytes = h->split_lds_bytes;
    if (workspace_bytes) *workspace_bytes = (int64_t)(h->split_doubles * sizeof(double));
    return GCSADMM_OK;
}

gcsadmm_status gcsadmm_unit_iterations(gcsadmm_handle h, int32_t *out, int32_t capacity, int32_t *count, void *stream)
{
    if (!h || !count) return GCSADMM_ERR_BAD_ARG;
    USE_DEVICE(h);
    const int *src = h->d_wave_iters ? h->d_wave_iters : h->d_wg_iters;
    const int n = h->d_wave_iters ? h->n_waves : (h->d_wg_iters ? h->n_wg : 0);
    *count = n;
    if (n == 0 || !out) return GCSADMM_OK;
    HIPCHK(h, hipStreamSynchronize((hipStream_t)stream));
    HIPCHK(h, hipMemcpy(out, src, sizeof(int) * (size_t)(n < capacity ? n : capacity), hipMemcpyDeviceToHost));
    return GCSADMM_OK;
}

} // extern "C"
