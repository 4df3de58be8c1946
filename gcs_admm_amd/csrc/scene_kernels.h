// scene_kernels.h -- the device side of polytope_lp.hip: the __global__ wrappers around the *_core.h headers (which have the rules and
// the contracts) with their argument and executor structs.  Included by polytope_lp.hip alone, the one translation unit of the scene.
#pragma once
#include <hip/hip_runtime.h>

#include "polytope_lp_core.h"
#include "box_sweep_core.h"
#include "point_locate_core.h"
#include "box_locate_core.h"
#include "point_project_core.h"
#include "segment_clip_core.h"
#include "scene_edit_core.h"
#include "query_graph_core.h"
#include "induced_graph_core.h"
#include "informed_core.h"
#include "informed_set_core.h"
#include "path_restrict_core.h"
#include "restrict_plan.h"

namespace gcsadmm_lp {

// ---- kernels (LDS: lam[maxm][64], dlam[maxm][64]) ----
template <int N>
__global__ __launch_bounds__(WAVE) void ball_kernel(Polys S, int count, const int *pa, const int *pb, const double *x0s,
                                                   int maxm, double tol, int early, double *out_w, unsigned char *out_flag, int *out_status)
{
    extern __shared__ double smem[];
    double *lam = smem, *dlam = smem + (size_t)maxm * WAVE;
    const int t = blockIdx.x * WAVE + threadIdx.x, lane = threadIdx.x;
    if (t >= count) return;
    const int p = pa ? pa[t] : t, q = pb ? pb[t] : -1;
    Rows<N, true> R(S, p, q);
    double w[N + 1], c[N + 1];
#pragma unroll
    for (int k = 0; k < N; ++k) c[k] = 0.0;
    c[N] = -1.0;
    ball_start<N>(R, x0s ? x0s + (size_t)p * N : nullptr, w);
    int iters = 0;
    const int st = lp_ipm<N, true>(R, c, w, lam, dlam, lane, early != 0, tol, &iters);
    if (out_w) {
#pragma unroll
        for (int k = 0; k <= N; ++k) out_w[(size_t)t * (N + 1) + k] = w[k];
    }
    if (out_flag) out_flag[t] = (st == 1) ? 1 : (st == 2 ? 0 : (w[N] >= -tol ? 1 : 0));
    if (out_status) out_status[t] = st;
}

template <int N>
// polytopes first .. first + count - 1; out_status counts from `first` (lo, hi and centers are the scene's arrays)
__global__ __launch_bounds__(WAVE) void bounds_kernel(Polys S, int first, int count, const double *centers, int maxm, double *lo, double *hi,
                                                     int *out_status)
{
    extern __shared__ double smem[];
    double *lam = smem, *dlam = smem + (size_t)maxm * WAVE;
    const int t = blockIdx.x * WAVE + threadIdx.x, lane = threadIdx.x;
    if (t >= count * 2 * N) return;
    const int p = first + t / (2 * N), j = t % (2 * N), k = j >> 1, upper = j & 1;
    double xk;
    const int st = bound_lp<N>(S, p, centers + (size_t)p * N, k, upper, lam, dlam, lane, xk, nullptr);
    (upper ? hi : lo)[(size_t)p * N + k] = xk;
    if (out_status) out_status[t] = st;
}

// ---- the resident scene's own kernels ----
// centres [P][n] and radii [P] out of the ball LPs' (x, r) records
__global__ void split_centres_kernel(const double *w, int n, int P, double *centers, double *radii)
{
    const int p = blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= P) return;
    for (int k = 0; k < n; ++k) centers[(size_t)p * n + k] = w[(size_t)p * (n + 1) + k];
    radii[p] = w[(size_t)p * (n + 1) + n];
}

// a side whose bounds LP did not converge is an interior iterate, a box that is too small: open it (status layout [P][n][(min, max)])
__global__ void open_failed_sides_kernel(const int *status, int n, int P, double *lo, double *hi)
{
    const long t = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= (long)P * 2 * n || status[t] >= 0) return;
    const long side = t >> 1;          // p * n + k
    if (t & 1) hi[side] = INFINITY;
    else lo[side] = -INFINITY;
}

// counts[0] = pairs flagged as overlapping, counts[1] = pairs whose LP reports status < 0: one add per wavefront and counter
__global__ void count_decisions_kernel(const unsigned char *flag, const int *status, long T, unsigned long long *counts)
{
    const long t = (long)blockIdx.x * blockDim.x + threadIdx.x;
    const unsigned long long over = __ballot(t < T && flag[t] != 0), undecided = __ballot(t < T && status[t] < 0);
    if ((threadIdx.x & (SWEEP_WAVE - 1)) == 0) {
        if (over) atomicAdd(&counts[0], (unsigned long long)__popcll(over));
        if (undecided) atomicAdd(&counts[1], (unsigned long long)__popcll(undecided));
    }
}

__global__ void first_lower_bounds_kernel(const double *lo, int n, int P, double *lo0)
{
    const int p = blockIdx.x * blockDim.x + threadIdx.x;
    if (p < P) lo0[p] = lo[(size_t)p * n];
}

__global__ void sweep_gather_kernel(const double *lo, const double *hi, const int *order, int n, int P, double *slo, double *shi)
{
    const int t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t < P) sweep_gather(lo, hi, order, n, P, t, slo, shi);
}

// one wavefront per box of the sweep order.  FILL = false: count[k] = pairs of box k; FILL = true: the same tests again, the pairs
// written from offset[k] on in window order.
template <int N, bool FILL>
__global__ __launch_bounds__(SWEEP_WAVE) void sweep_kernel(SortedBoxes B, double pad, int *count, const long long *offset, int *pair_a, int *pair_b)
{
    const int k = blockIdx.x, lane = threadIdx.x;
    SweepBox<N> bk;
    sweep_load_box<N>(B, k, pad, bk);
    const int end = sweep_window_end(B.lo, B.P, bk.hip[0]);
    const int ok = FILL ? B.order[k] : 0;
    long long pos = FILL ? offset[k] : 0;
    int total = 0;
    for (int j0 = k + 1; j0 < end; j0 += SWEEP_WAVE) {
        const int j = j0 + lane;
        const bool hit = j < end && sweep_test<N>(B, bk, j, pad);
        const unsigned long long mask = __ballot(hit);
        if (FILL) {
            if (hit) sweep_store_pair(pair_a, pair_b, pos + sweep_rank(mask, lane), ok, B.order[j]);
            pos += sweep_hits(mask);
        } else {
            total += sweep_hits(mask);
        }
    }
    if (!FILL && lane == 0) count[k] = total;
}

// ---- path restrictions on the resident regions ----
// executor of path_restrict_solve: one wavefront; reductions by shuffles in a fixed order (bit-reproducible, and the same whatever
// else the launch holds); the barrier first waits for the wavefront's global accesses (the phases hand values over through the
// workspace: vertex_wg.h WG_VM has the reason)
struct RestrictExec {
    __device__ __forceinline__ int tid() const { return (int)threadIdx.x; }
    __device__ __forceinline__ int nthreads() const { return gcsadmm_k::RESTRICT_THREADS; }
    __device__ __forceinline__ int task(int u, int) const { return u; }
    __device__ __forceinline__ void sync()
    {
        asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");
        __syncthreads();
    }
    __device__ __forceinline__ void reduce3(double &mn, double &s1, double &s2)
    {
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) {
            mn = fmin(mn, __shfl_xor(mn, off, 64));
            s1 += __shfl_xor(s1, off, 64);
            s2 += __shfl_xor(s2, off, 64);
        }
    }
};

struct RestrictArgs {
    const int *poly_ptr;
    const double *A, *b;
    const int *path_ptr, *path_poly, *row_prefix;
    const long long *ws_off;
    double *ws;
    const double *start;
    double *points, *cost;
    int *iterations, *status;
    double tol;
    int max_iter, num_paths;
};

template <int N>
__global__ __launch_bounds__(gcsadmm_k::RESTRICT_THREADS) void path_restrict_kernel(RestrictArgs a)
{
    __shared__ gcs_restrict::PathShared<N> sh;
    const int p = (int)blockIdx.x;
    if (p >= a.num_paths) return;
    const int first = a.path_ptr[p];
    gcs_restrict::PathProblem pr;
    pr.k = a.path_ptr[p + 1] - first;
    pr.poly = a.path_poly + first;
    pr.rowp = a.row_prefix + first + 2 * (size_t)p;
    pr.poly_ptr = a.poly_ptr; pr.A = a.A; pr.b = a.b;
    pr.start = a.start + (size_t)(first + p) * N;
    pr.points = a.points + (size_t)(first + p) * N;
    pr.tol = a.tol; pr.max_iter = a.max_iter;
    RestrictExec ex;
    double cost;
    int iterations;
    const int st = gcs_restrict::path_restrict_solve<N>(ex, pr, a.ws + a.ws_off[p], sh, &cost, &iterations);
    if (threadIdx.x == 0) { a.cost[p] = cost; a.iterations[p] = iterations; a.status[p] = st; }
}

// ---- the regions under query points ----
struct LocateArgs {
    LocateRegions R;
    const double *points;      // [num_points][N]
    double margin;             // eps + 2 tol
    int first_point;           // blockIdx.y counts from here (one launch takes at most 65 535 points)
    long long chunks, limit;   // chunks of the P regions; length of the list
    int *count;                // [num_points][chunks]
    const long long *offset;   // [num_points][chunks]
    int *hit_region;
    unsigned char *hit_class;
};

// one 64-lane workgroup per (chunk of regions, point), one region per lane.  FILL = false: count[point][chunk] = regions of the chunk
// that are not OUT; FILL = true: the same tests again, the hits written from offset[point][chunk] on in region order.
template <int N, bool FILL>
__global__ __launch_bounds__(LOCATE_WAVE) void locate_kernel(LocateArgs a)
{
    const long long chunk = blockIdx.x, q = (long long)a.first_point + blockIdx.y;
    const int lane = threadIdx.x;
    double p[N];
#pragma unroll
    for (int k = 0; k < N; ++k) p[k] = a.points[(size_t)q * N + k];      // the same address in every lane
    const size_t cell = (size_t)(q * a.chunks + chunk);
    long long pos = FILL ? a.offset[cell] : 0;
    int total = 0;
    for (int stride = 0; stride < LOCATE_CHUNK / LOCATE_WAVE; ++stride) {
        const int region = locate_region(a.R.P, chunk, stride, lane);
        const int cls = locate_lane<N>(a.R, region, p, a.margin);
        const unsigned long long mask = __ballot(cls != LOCATE_OUT);
        if (FILL) {
            locate_store(a.hit_region, a.hit_class, pos, a.limit, mask, lane, region, cls);
            pos += locate_hits(mask);
        } else {
            total += locate_hits(mask);
        }
    }
    if (!FILL && lane == 0) a.count[cell] = total;
}

// ---- the regions that query boxes meet (box_locate_core.h) ----
struct LocateBoxArgs {
    LocateRegions R;
    const double *boxes;       // [num_boxes][2 N]: the centre, then the half-widths + 2 tol (locate_box_prepare)
    int first_box;             // blockIdx.y counts from here (one launch takes at most 65 535 boxes)
    long long chunks, limit;   // chunks of the P regions; length of the list
    int *count;                // [num_boxes][chunks]
    const long long *offset;   // [num_boxes][chunks]
    int *hit_region;
    unsigned char *hit_class;
};

// locate_kernel's shape with a box in the place of the point: one 64-lane workgroup per (chunk of regions, box), one region per lane,
// a count pass (FILL = false) and a fill pass that runs the same tests again and writes the hits from offset[box][chunk] on
template <int N, bool FILL>
__global__ __launch_bounds__(LOCATE_WAVE) void locate_box_kernel(LocateBoxArgs a)
{
    const long long chunk = blockIdx.x, q = (long long)a.first_box + blockIdx.y;
    const int lane = threadIdx.x;
    double c[N], hw[N];
#pragma unroll
    for (int k = 0; k < N; ++k) {      // the same addresses in every lane
        c[k] = a.boxes[(size_t)q * 2 * N + k];
        hw[k] = a.boxes[(size_t)q * 2 * N + N + k];
    }
    const size_t cell = (size_t)(q * a.chunks + chunk);
    long long pos = FILL ? a.offset[cell] : 0;
    int total = 0;
    for (int stride = 0; stride < LOCATE_CHUNK / LOCATE_WAVE; ++stride) {
        const int region = locate_region(a.R.P, chunk, stride, lane);
        const int cls = locate_box_lane<N>(a.R, region, c, hw);
        const unsigned long long mask = __ballot(cls != LOCATE_OUT);
        if (FILL) {
            locate_store(a.hit_region, a.hit_class, pos, a.limit, mask, lane, region, cls);
            pos += locate_hits(mask);
        } else {
            total += locate_hits(mask);
        }
    }
    if (!FILL && lane == 0) a.count[cell] = total;
}

// ---- the nearest regions of query points (point_project_core.h) ----
struct ProjectArgs {
    LocateRegions R;
    const double *points;      // [num_points][N]
    const double *radius;      // [num_points], +inf allowed
    int first_point;           // blockIdx.y counts from here (one launch takes at most 65 535 points)
    long long chunks, limit;   // chunks of the P regions; length of the list
    int *count;                // [num_points][chunks]
    const long long *offset;   // [num_points][chunks]
    int *hit_region;
    unsigned char *hit_class;
};

// locate_kernel's shape with the candidate test of a projection: one 64-lane workgroup per (chunk of regions, point), one region per
// lane, a count pass (FILL = false) and a fill pass that runs the same tests again and writes the candidates from offset[point][chunk] on
template <int N, bool FILL>
__global__ __launch_bounds__(LOCATE_WAVE) void project_list_kernel(ProjectArgs a)
{
    const long long chunk = blockIdx.x, q = (long long)a.first_point + blockIdx.y;
    const int lane = threadIdx.x;
    double p[N];
#pragma unroll
    for (int k = 0; k < N; ++k) p[k] = a.points[(size_t)q * N + k];      // the same address in every lane
    const double radius = a.radius[q];
    const size_t cell = (size_t)(q * a.chunks + chunk);
    long long pos = FILL ? a.offset[cell] : 0;
    int total = 0;
    for (int stride = 0; stride < LOCATE_CHUNK / LOCATE_WAVE; ++stride) {
        const int region = locate_region(a.R.P, chunk, stride, lane);
        const int cls = project_lane<N>(a.R, region, p, radius);
        const unsigned long long mask = __ballot(cls != PROJECT_OUT);
        if (FILL) {
            locate_store(a.hit_region, a.hit_class, pos, a.limit, mask, lane, region, cls);
            pos += locate_hits(mask);
        } else {
            total += locate_hits(mask);
        }
    }
    if (!FILL && lane == 0) a.count[cell] = total;
}

struct ProjectSolveArgs {
    LocateRegions R;
    const double *points, *radius;
    const long long *hit_ptr;  // [num_points + 1]
    long long num_points, total;
    const int *hit_region;
    int max_iter;
    long long first;           // blockIdx.x counts workgroups from this list entry on
    ProjectOut out;
};

// one lane per candidate pair in list order, 64 pairs per workgroup; the working set of a lane stays in its registers
template <int N>
__global__ __launch_bounds__(PROJECT_LANES) void project_solve_kernel(ProjectSolveArgs a)
{
    const long long t = a.first + (long long)blockIdx.x * PROJECT_LANES + threadIdx.x;
    if (t < a.total) project_entry<N>(a.R, a.points, a.radius, a.hit_ptr, a.num_points, a.hit_region, a.max_iter, t, a.out);
}

// ---- the regions a segment runs through, and whether they cover it (segment_clip_core.h) ----
struct ClipArgs {
    LocateRegions R;
    const double *from, *to;   // [num_segments][N] each
    double tol;
    int first_segment;         // blockIdx.y counts from here (one launch takes at most 65 535 segments)
    long long chunks, limit;   // chunks of the P regions; length of the list
    int *count;                // [num_segments][chunks]
    const long long *offset;   // [num_segments][chunks]
    int *hit_region;
    unsigned char *hit_class;
    double *hit_in, *hit_out;  // the span of every hit
};

// locate_kernel's shape with a segment in the place of the point: one 64-lane workgroup per (chunk of regions, segment), one region per
// lane, a count pass (FILL = false) and a fill pass that runs the same tests again and writes the hits and their spans from
// offset[segment][chunk] on
template <int N, bool FILL>
__global__ __launch_bounds__(LOCATE_WAVE) void segment_clip_kernel(ClipArgs a)
{
    const long long chunk = blockIdx.x, q = (long long)a.first_segment + blockIdx.y;
    const int lane = threadIdx.x;
    double p[N], e[N], d[N];
#pragma unroll
    for (int k = 0; k < N; ++k) {      // the same addresses in every lane
        p[k] = a.from[(size_t)q * N + k];
        e[k] = a.to[(size_t)q * N + k];
    }
    clip_direction<N>(p, e, d);
    const size_t cell = (size_t)(q * a.chunks + chunk);
    long long pos = FILL ? a.offset[cell] : 0;
    int total = 0;
    for (int stride = 0; stride < LOCATE_CHUNK / LOCATE_WAVE; ++stride) {
        const int region = locate_region(a.R.P, chunk, stride, lane);
        double t_in = 0.0, t_out = 0.0;
        const int cls = clip_lane<N>(a.R, region, p, d, a.tol, &t_in, &t_out);
        const unsigned long long mask = __ballot(cls != CLIP_OUT);
        if (FILL) {
            clip_store(a.hit_region, a.hit_class, a.hit_in, a.hit_out, pos, a.limit, mask, lane, region, cls, t_in, t_out);
            pos += locate_hits(mask);
        } else {
            total += locate_hits(mask);
        }
    }
    if (!FILL && lane == 0) a.count[cell] = total;
}

struct ChainArgs {
    const long long *hit_ptr;      // [num_segments + 1]
    const double *hit_in, *hit_out;
    long long first_segment;       // blockIdx.x counts from here
    int *status;                   // [num_segments] COVER_COVERED / COVER_GAP
    double *reach;                 // [num_segments]
    int *chain_len;                // [num_segments]
    int *chain_hit;                // [length of the list]: the chain of segment q from hit_ptr[q] on, as positions in the list
};

// the cover test: one 64-lane wavefront per segment.  A step is chain_lane_best over the hits lane, lane + 64, ... and one butterfly of
// shuffles on (t_out, position), after which every lane holds the same best: no LDS, no barrier, no atomics.  The span at position
// `lane` stays in two registers across the steps
__global__ __launch_bounds__(LOCATE_WAVE) void segment_chain_kernel(ChainArgs a)
{
    const long long q = a.first_segment + blockIdx.x;
    const int lane = threadIdx.x;
    const long long first = a.hit_ptr[q];
    const int count = (int)(a.hit_ptr[q + 1] - first);
    const double *t_in = a.hit_in + first, *t_out = a.hit_out + first;
    const double first_in = lane < count ? t_in[lane] : 0.0, first_out = lane < count ? t_out[lane] : 0.0;
    double cur = 0.0;
    int len = 0, status = COVER_COVERED;
    while (cur < 1.0) {
        double best_out;
        int best_pos;
        chain_lane_best(t_in, t_out, count, lane, first_in, first_out, cur, &best_out, &best_pos);
#pragma unroll
        for (int off = LOCATE_WAVE / 2; off > 0; off >>= 1) {
            const double other_out = __shfl_xor(best_out, off);
            const int other_pos = __shfl_xor(best_pos, off);
            if (chain_better(other_out, other_pos, best_out, best_pos)) { best_out = other_out; best_pos = other_pos; }
        }
        if (best_pos == CHAIN_NONE || len >= count) { status = COVER_GAP; break; }      // (len < count always: a hit is taken once)
        if (lane == 0) a.chain_hit[first + len] = (int)(first + best_pos);
        ++len;
        cur = best_out;
    }
    if (lane == 0) { a.status[q] = status; a.reach[q] = cur; a.chain_len[q] = len; }
}

// ---- edits of a decided scene (scene_edit_core.h) ----
__global__ void edit_rank_kernel(EditRanks E)
{
    const int t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t < E.P + E.K) edit_rank(E, t);
}

// one 64-lane workgroup per (chunk of targets, sweeping box), one target per lane.  FILL = false: count[box][chunk] = targets of the
// chunk that pair with the box; FILL = true: the same tests again, the pairs written from offset[box][chunk] on in target order.
template <int N, bool FILL>
__global__ __launch_bounds__(SWEEP_WAVE) void cross_kernel(CrossSide c, double pad)
{
    const long long chunk = blockIdx.x;
    const int k = c.first + (int)blockIdx.y, lane = threadIdx.x;
    SweepBox<N> bk;
    sweep_load_box<N>(c.S, k, pad, bk);
    int w0, w1;
    cross_window<N>(c, k, bk, w0, w1);
    const size_t cell = (size_t)(c.cell0 + (long long)k * c.chunks + chunk);
    int total = 0;
    if (cross_chunk_live(chunk, w0, w1)) {      // (the same in every lane)
        const int re = cross_sweeper_rank(c, k, w0);
        long long pos = FILL ? c.offset[cell] : 0;
        for (int stride = 0; stride < EDIT_CHUNK / SWEEP_WAVE; ++stride) {
            int j;
            const bool hit = cross_hit<N>(c, bk, w0, w1, chunk, stride, lane, pad, j);
            const unsigned long long mask = __ballot(hit);
            if (FILL) {
                if (hit) cross_store(c, pos + sweep_rank(mask, lane), re, j);
                pos += sweep_hits(mask);
            } else {
                total += sweep_hits(mask);
            }
        }
    }
    if (!FILL && lane == 0) c.count[cell] = total;
}

__global__ void merge_count_kernel(EditMerge m)
{
    const int r = blockIdx.x * blockDim.x + threadIdx.x;
    if (r < m.P + m.K) merge_count(m, r);
}
__global__ void merge_move_old_kernel(EditMerge m)
{
    const long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (t < m.T_old) merge_move_old(m, t);
}
__global__ void merge_move_new_kernel(EditMerge m)
{
    const long long x = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (x < m.T_new) merge_move_new(m, x);
}

template <bool FILL> __global__ void remove_segment_kernel(EditRemove e)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < e.P) remove_segment<FILL>(e, i);
}
template <class V> __global__ void compact_rows_kernel(const V *src, V *dst, const int *newidx, int width, int P)
{
    const int p = blockIdx.x * blockDim.x + threadIdx.x;
    if (p < P) remove_compact_row(src, dst, newidx, width, p);
}
__global__ void compact_polys_kernel(const int *ptr, const int *new_ptr, const int *newidx, int n, int P, const double *A, const double *b,
                                     const double *nrm, double *A2, double *b2, double *nrm2)
{
    const int p = blockIdx.x * blockDim.x + threadIdx.x;
    if (p < P) remove_compact_poly(ptr, new_ptr, newidx, n, p, A, b, nrm, A2, b2, nrm2);
}

// ---- the region graph and the query graphs of a decided scene (query_graph_core.h) ----
__global__ void region_count_kernel(RegionBuild g)
{
    const long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (t < g.T) region_count(g, t);
}
__global__ void region_scatter_kernel(RegionBuild g)
{
    const long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (t < g.T) region_scatter(g, t);
}
__global__ void region_place_kernel(RegionBuild g, long long E)
{
    const long long p = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (p < E) region_place(g, p);
}
__global__ void region_reverse_kernel(RegionBuild g, long long E)
{
    const long long p = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (p < E) region_reverse(g, p);
}

struct QueryGraphArgs {
    RegionGraph g;
    QueryBatch q;             // device copies of the caller's arrays
    QueryArrays out;          // the chunk's buffers: they begin with query `first`
    int first;                // blockIdx.y counts queries from here
    long long items;          // the most work items of one query of the call
};
// one thread per work item of one query (query_item): blockIdx.y the query of the chunk, blockIdx.x * 256 + threadIdx.x the item
__global__ __launch_bounds__(256) void query_graph_kernel(QueryGraphArgs a)
{
    const int i = a.first + (int)blockIdx.y;
    const long long x = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (x >= a.items) return;
    query_item(a.g, query_terms(a.q, i), query_arrays(a.out, a.q, a.g.P, a.first, i), x);
}

// ---- the query graphs of a batch on each query's kept regions (induced_graph_core.h) ----
struct InducedArgs {
    RegionGraph g;                  // the scene's
    const InducedQuery *table;      // [queries of the chunk]: blockIdx.x (count, build) or blockIdx.y (query) indexes it
    QueryBatch q;                   // device copies of the caller's arrays, scene indices in term_region
    int *term_new;                  // the hit lists renumbered, laid out as term_region
    int first;                      // the chunk's first query
    int *sizes;                     // [queries of the chunk][INDUCED_SIZES]
};
// One workgroup per query: the flags in tiles of 256, each lane the region of its place in the tile.
__global__ __launch_bounds__(INDUCED_TILE) void induced_count_kernel(InducedArgs a)
{
    __shared__ int part[INDUCED_TILE / INDUCED_WAVE];
    const InducedQuery q = a.table[blockIdx.x];
    const int P = a.g.P, t = (int)threadIdx.x;
    TileCarry below;
    InducedCount sum{0, 0};
    for (int base = 0; base < P; base += INDUCED_TILE) {      // (the same trips in every lane: the scan has barriers)
        const int r = base + t, flag = induced_flag(q, P, r);
        int total;
        const int within = induced_tile_scan(flag, part, total);
        if (r < P) induced_number(a.g, q, r, flag, below.at(within), sum);
        below.next(total);
    }
    int edges, ranks;
    induced_tile_scan(sum.edges, part, edges);
    induced_tile_scan(sum.ranks, part, ranks);
    if (t == 0) {
        int *z = a.sizes + (size_t)INDUCED_SIZES * blockIdx.x;
        z[0] = below.sum; z[1] = edges; z[2] = ranks;
    }
}
// One workgroup per query: the kept rows in tiles of 256, each lane the row of its place in the tile; then, behind a barrier that
// first waits for the wavefront's stores (region_path_kernel has the form), the reverse edges from the ranks the other lanes wrote.
__global__ __launch_bounds__(INDUCED_TILE) void induced_build_kernel(InducedArgs a)
{
    __shared__ int part[INDUCED_TILE / INDUCED_WAVE];
    const InducedQuery q = a.table[blockIdx.x];
    const int i = a.first + (int)blockIdx.x, t = (int)threadIdx.x, kept = q.kept_count;
    TileCarry first, ranks;
    for (int base = 0; base < kept; base += INDUCED_TILE) {
        const int j = base + t;
        int edges, full;
        const int e_within = induced_tile_scan(j < kept ? q.deg[j] : 0, part, edges);
        const int f_within = induced_tile_scan(j < kept ? induced_full_degree(a.g, q, j) : 0, part, full);
        if (j < kept) induced_row(a.g, q, j, first.at(e_within), ranks.at(f_within));
        first.next(edges); ranks.next(full);
    }
    if (t == 0) q.row_ptr[kept] = first.sum;
    for (int k = t, hits = induced_hits(a.q, i); k < hits; k += INDUCED_TILE) induced_term(a.q, i, q.newidx, a.term_new, k);
    asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");
    __syncthreads();
    for (int j = t; j < kept; j += INDUCED_TILE) induced_reverse(a.g, q, j);
}
struct InducedGraphArgs {
    const InducedQuery *table;      // [queries of the chunk]
    QueryBatch q;                   // device copies; term_region holds the renumbered lists
    const long long *vertex_off;    // [B + 1]
    QueryArrays out;                // the chunk's buffers: they begin with query `first`
    int first;
};
// query_graph_kernel with the region graph and the item count of each query from the table (the grid covers the most items of one)
__global__ __launch_bounds__(256) void induced_graph_kernel(InducedGraphArgs a)
{
    const int i = a.first + (int)blockIdx.y;
    const long long x = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    const RegionGraph g = induced_region_graph(a.table[blockIdx.y]);
    const QueryTerms t = query_terms(a.q, i);
    if (x >= query_items(g, t.a, t.b)) return;
    query_item(g, t, induced_arrays(a.out, a.q, a.vertex_off, a.first, i), x);
}

// ---- the informed region set of a query (informed_core.h) ----
__global__ void region_weight_kernel(const double *centers, int n, const int *tail, const int *head, long long E, double *w)
{
    const long long p = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (p < E) w[p] = informed_weight(centers, n, tail, head, p);
}

struct PathArgs {
    PathGraph g;
    const double *points;           // [2 B][n]: the starts, then the goals
    const long long *term_ptr;      // [2 B + 1]
    const int *term_region;
    int B, first, max_len;          // blockIdx.x counts queries from `first`
    double *d;                      // [queries of the chunk][P]
    int *path_region, *path_len, *status;      // [B][max_len], [B], [B]
    double *path_cost;              // [B]
};
// One workgroup per query.  Lane t owns the vertices t, t + 256, ...: it alone writes their entries of d, by plain stores, from what
// it reads of its rows' neighbours, in place.  A round ends at a barrier that first waits for the wavefront's global accesses
// (RestrictExec::sync has the form), so the next round reads what this one wrote; `changed` carries whether any lane lowered a value
// across it -- three flags in turn, so that the one of round r + 2 is cleared between barriers r and r + 1, when nobody reads or sets
// it.  A round that changes nothing has read final values only: the fixed point, whatever order the lanes ran in.  At most P rounds.
__global__ __launch_bounds__(PATH_THREADS) void region_path_kernel(PathArgs a)
{
    __shared__ int changed[3];
    const int i = a.first + (int)blockIdx.x, t = (int)threadIdx.x, P = a.g.P, n = a.g.n;
    if (i >= a.B) return;
    PathQuery q;
    q.s = a.points + (size_t)i * n; q.g = a.points + (size_t)(a.B + i) * n;
    q.rs = a.term_region + a.term_ptr[i]; q.a = (int)(a.term_ptr[i + 1] - a.term_ptr[i]);
    q.rt = a.term_region + a.term_ptr[a.B + i]; q.b = (int)(a.term_ptr[a.B + i + 1] - a.term_ptr[a.B + i]);
    double *d = a.d + (size_t)blockIdx.x * P;
    auto sync = [] {
        asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");
        __syncthreads();
    };
    for (int v = t; v < P; v += PATH_THREADS) d[v] = informed_init(a.g, q, v);
    if (t < 3) changed[t] = 0;
    sync();
    for (int round = 0; round < P; ++round) {
        bool fell = false;
        for (int v = t; v < P; v += PATH_THREADS) fell |= informed_relax(a.g, d, v);
        if (fell) changed[round % 3] = 1;
        sync();
        if (!changed[round % 3]) break;      // (the same in every lane)
        if (t == 0) changed[(round + 2) % 3] = 0;
    }
    if (t == 0)
        a.status[i] = informed_backtrack(a.g, q, d, a.max_len, a.path_region + (size_t)i * a.max_len, a.path_len + i, a.path_cost + i);
}

struct KeepArgs {
    int P, n, B, first;             // blockIdx.y counts queries from `first`
    const double *lo, *hi;          // [P][n]
    const double *points, *bound;   // [2 B][n], [B]
    double pad;
    unsigned char *keep;            // [B][P]
};
// one thread per (query, region)
__global__ __launch_bounds__(256) void informed_keep_kernel(KeepArgs a)
{
    const int i = a.first + (int)blockIdx.y, r = (int)(blockIdx.x * blockDim.x + threadIdx.x);
    if (r >= a.P) return;
    const double lb = informed_lower_bound(a.points + (size_t)i * a.n, a.points + (size_t)(a.B + i) * a.n, a.lo + (size_t)r * a.n, a.hi + (size_t)r * a.n, a.n, a.pad);
    a.keep[(size_t)i * a.P + r] = informed_keep(lb, a.bound[i]) ? 1 : 0;
}

// ---- the informed region set of a query between start and goal sets (informed_set_core.h) ----
struct SetPathArgs {
    PathGraph g;
    const double *lo, *hi;          // [2 B][n] each: the start boxes, then the goal boxes
    const long long *term_ptr;      // [2 B + 1]
    const int *term_region;
    int B, first, max_len;          // blockIdx.x counts queries from `first`
    double *d;                      // [queries of the chunk][P]
    int *path_region, *path_len, *status;      // [B][max_len], [B], [B]
    double *path_cost;              // [B]
};
// region_path_kernel's rounds (one workgroup per query, lane t owns the vertices t, t + 256, ..., the same round boundary and the same
// three flags) under the bound of informed_set_core.h.  `bound` holds the bits of U: a non-negative double or +inf, which order as
// their bits do, so the cell takes an unsigned minimum and only ever falls -- it needs no clearing and no rotation.  Behind a round's
// barrier the lanes stride over the goal list and fold the goal costs of what that round left in d into the cell; a lane reads the
// cell once, ahead of its relaxations, and may still see the value of the round before: that one was the goal cost of a d already
// written too, and only admits more.
__global__ __launch_bounds__(PATH_THREADS) void terminal_set_path_kernel(SetPathArgs a)
{
    __shared__ int changed[3];
    __shared__ unsigned long long bound;
    const int i = a.first + (int)blockIdx.x, t = (int)threadIdx.x, P = a.g.P;
    if (i >= a.B) return;
    const SetQuery q = set_query(a.lo, a.hi, a.term_ptr, a.term_region, a.B, a.g.n, i);
    double *d = a.d + (size_t)blockIdx.x * P;
    auto sync = [] {
        asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");
        __syncthreads();
    };
    // (the lane's first goal region and that region's distance to G do not change from round to round: a fold is then one load of d
    // for all but the lists longer than the lanes)
    const int r0 = t < q.b ? q.rt[t] : -1;
    const double g0 = r0 >= 0 ? set_point_distance(a.g.centers + (size_t)r0 * a.g.n, q.glo, q.ghi, a.g.n) : 0.0;
    auto lower = [&](double c) {
        if (set_lowers(c, __longlong_as_double((long long)bound))) atomicMin(&bound, (unsigned long long)__double_as_longlong(c));
    };
    auto fold = [&] {
        if (r0 >= 0) lower(d[r0] + g0);
        for (int j = t + PATH_THREADS; j < q.b; j += PATH_THREADS) lower(set_goal_cost(a.g, q, d, q.rt[j]));
    };
    for (int v = t; v < P; v += PATH_THREADS) d[v] = set_init(a.g, q, v);
    if (t < 3) changed[t] = 0;
    if (t == 0) bound = (unsigned long long)__double_as_longlong(INFINITY);
    sync();
    fold();
    for (int round = 0; round < P; ++round) {
        const double U = __longlong_as_double((long long)bound);
        bool fell = false;
        for (int v = t; v < P; v += PATH_THREADS) fell |= set_relax(a.g, d, v, U);
        if (fell) changed[round % 3] = 1;
        sync();
        if (!changed[round % 3]) break;      // (the same in every lane)
        if (t == 0) changed[(round + 2) % 3] = 0;
        fold();
    }
    if (t == 0)
        a.status[i] = set_backtrack(a.g, q, d, a.max_len, a.path_region + (size_t)i * a.max_len, a.path_len + i, a.path_cost + i);
}

struct SetKeepArgs {
    int P, n, B, first;             // blockIdx.y counts queries from `first`
    const double *lo, *hi;          // [P][n]: the resident boxes
    const double *tlo, *thi;        // [2 B][n] each: the start boxes, then the goal boxes
    const double *bound;            // [B]
    double pad;
    unsigned char *keep;            // [B][P]
};
// one thread per (query, region)
__global__ __launch_bounds__(256) void terminal_set_keep_kernel(SetKeepArgs a)
{
    const int i = a.first + (int)blockIdx.y, r = (int)(blockIdx.x * blockDim.x + threadIdx.x);
    if (r >= a.P) return;
    const SetQuery q = set_query(a.tlo, a.thi, nullptr, nullptr, a.B, a.n, i);
    a.keep[(size_t)i * a.P + r] = informed_keep(set_lower_bound(q, a.lo + (size_t)r * a.n, a.hi + (size_t)r * a.n, a.n, a.pad), a.bound[i]) ? 1 : 0;
}

} // namespace gcsadmm_lp
