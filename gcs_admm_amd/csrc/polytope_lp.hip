// polytope_lp.hip -- batched tiny linear programs for graph construction at scale (gfx950)
//
// The reference builds the graph with one LP feasibility solve per ordered pair of regions through
// Drake/MOSEK (utils.py:31-82: build_graph -> check_overlap, :49-65) -- |V|^2 host solves.  Here one
// lane solves one LP with a primal-dual interior-point method (Mehrotra predictor-corrector, normal
// equations of size n+1 <= 7, f64), 64 LPs per wavefront, rows streamed from the polytope CSR:
//
//   centres  : max r  s.t.  a_i x + r |a_i| <= b_i                  (Chebyshev centre of one polytope:
//                                                                    the interior point the vertex kernel
//                                                                    centres its sub-problem on)
//   overlaps : the same LP over the rows of two polytopes; the pair intersects iff r* >= -tol
//              (closed sets: touching counts, as it does for an LP feasibility solve)
//   bounds   : min / max x_k over one polytope, from its centre      (axis-aligned bounding boxes for the
//                                                                    broad phase: sort-and-sweep, on the host
//                                                                    in scene.py or here in sweep_kernel)
//
// Per lane: the unknowns, the (n+1)^2 normal matrix and its Cholesky factor live in registers; the row
// duals and their directions sit in LDS as [row][lane] (conflict-free); every Newton iteration makes five
// passes over the rows.  An overlap LP stops as soon as the current (always strictly feasible) iterate has
// r > 0, or the dual bound proves r* < -tol.
//
// A gcsadmm_scene keeps the polytopes, the centres, the boxes and the pair list on the device from the first LP to the last; its
// broad phase is sweep_kernel (box_sweep_core.h has the contract), so that only counts and the final pair list cross to the host.
//
// The resident regions also serve the step after the loop: path_restrict_kernel solves the convex restriction along fixed paths
// (path_restrict_core.h: one 64-lane workgroup per path, a block-tridiagonal Newton system factored along the path), on the offsets
// and sizes restrict_plan.h decides.
//
// And the queries on a scene whose graph is decided: locate_kernel lists the regions under each start and goal point
// (point_locate_core.h has the rule), so that a query costs no region-region LP.
//
// A decided scene can grow and shrink (gcsadmm_scene_add_regions, gcsadmm_scene_remove_regions; scene_edit_core.h has the contract):
// the LPs of the new regions and of their pairs alone, cross_kernel for the new boxes against all boxes, and a merge that leaves the
// pair list a scene built from scratch on the edited set would have.
// The query graphs of a batch are assembled here as well (gcsadmm_scene_build_region_graph, gcsadmm_scene_query_graphs;
// query_graph_core.h has the contract): the region graph from the resident pair list without a sort, then one kernel that writes every
// entry of every query graph's index arrays from its closed form.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <new>
#include <optional>
#include <string>
#include <vector>

#include "gcsadmm.h"
#include "hip_owners.h"
#include "step_args.h"      // dispatch_dim

#include "polytope_lp_core.h"
#include "box_sweep_core.h"
#include "point_locate_core.h"
#include "scene_edit_core.h"
#include "query_graph_core.h"
#include "path_restrict_core.h"
#include "restrict_plan.h"

// the calling thread's last failure (gcsadmm_polytope_last_error)
static thread_local std::string g_err;
#define LPCHK(call)                                                                                  \
    do {                                                                                             \
        hipError_t e_ = (call);                                                                      \
        if (e_ != hipSuccess) {                                                                      \
            g_err = std::string(#call) + ": " + hipGetErrorString(e_);                               \
            return GCSADMM_ERR_HIP;                                                                  \
        }                                                                                            \
    } while (0)

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

} // namespace gcsadmm_lp

using namespace gcsadmm_lp;

// The scene: everything graph construction computes stays in these buffers until it is read.  A gcsadmm_scene holds one from create
// to destroy (read: gcsadmm_scene_read_pairs); a batch call (gcsadmm_polytope_*) holds one on its stack, with the buffers of its stage.
struct gcsadmm_scene_s {
    int n = 0, P = 0, device = 0;
    int maxm = 0;                                      // most rows of one polytope
    DevBuf<int> ptr;                                   // the polytopes: CSR, rows, right-hand sides, norms of the rows (S points at them)
    DevBuf<double> A, b, nrm;
    std::vector<int> h_ptr;                            // the CSR offsets on the host too (a resident scene's: restrict_plan.h reads them)
    Polys S{};
    DevBuf<double> w, cen, rad;                        // centre LPs: (x, r) records, centres [P][n], radii,
    DevBuf<int> st_c;                                  //   statuses
    DevBuf<double> lo, hi;                             // boxes [P][n]
    DevBuf<int> st_b;                                  //   and the statuses of their LPs [P][n][2]
    DevBuf<double> lo0, slo, shi;                      // sweep: first lower bounds, sorted boxes [n][P],
    DevBuf<int> order, count;                          //   sort order, counts,
    DevBuf<long long> offset;                          //   offsets
    DevBuf<int> pa, pb, st_o;                          // pair list with the narrow phase's statuses,
    DevBuf<unsigned char> flag;                        //   flags
    DevBuf<unsigned long long> counts;                 //   and the two counts of them
    long long T = 0;
    bool have_centers = false, have_boxes = false, have_pairs = false, have_overlaps = false;
    DevBuf<double> q_points;                           // queries (kept and grown from call to call): the points [num_points][n],
    DevBuf<int> q_count;                               //   counts and
    DevBuf<long long> q_offset;                        //   offsets per (point, chunk),
    DevBuf<int> hit_region;                            //   the hit list
    DevBuf<unsigned char> hit_class;
    std::vector<int64_t> hit_ptr;                      //   and its segments per point (host: the scan runs there)
    bool have_hits = false;
    DevBuf<long long> g_row_ptr;                       // region graph of the decided pairs (query_graph_core.h): rows [P + 1],
    DevBuf<int> g_tail, g_head, g_rev;                 //   edges by (tail, head) and the id of each one's opposite edge
    long long g_edges = 0;
    bool have_graph = false;                           //   (an edit or a new narrow phase ends it)
    DevBuf<long long> qg_term_ptr, qg_edge_off;        // query graphs (kept and grown from call to call): the caller's arrays
    DevBuf<int> qg_term_region;
    DevBuf<unsigned char> qg_st;
    DevBuf<int> qg_edge_tail, qg_edge_head, qg_inc_ptr, qg_inc_edge, qg_inc_out, qg_edge_inc_tail, qg_edge_inc_head;      //   one chunk of results
};

namespace {

constexpr int TB = 256;      // threads per block of the element-wise helpers
inline unsigned blocks_of(long count) { return (unsigned)((count + TB - 1) / TB); }

// f(std::integral_constant<int, N>) for the scene's n (upload_scene admits 1..8 only)
template <class F> int for_dim(int n, F &&f)
{
    int rc = GCSADMM_ERR_UNSUPPORTED;
    gcsadmm_k::dispatch_dim<1, 2, 3, 4, 5, 6, 7, 8>(n, [&](auto N) { rc = f(N); });
    return rc;
}

int guard_status(const DeviceGuard &guard)
{
    if (guard.err == hipSuccess) return GCSADMM_OK;
    g_err = std::string("hipSetDevice: ") + hipGetErrorString(guard.err);
    return GCSADMM_ERR_HIP;
}
// entry of every call on a resident scene: the scene's device for the call, the caller's back on return
#define USE_SCENE(s)                                                                                 \
    if (!(s)) { g_err = "null scene"; return GCSADMM_ERR_BAD_ARG; }                                  \
    DeviceGuard device_guard_((s)->device);                                                          \
    if (int rc_ = guard_status(device_guard_)) return rc_

// Checks the polytopes on the host; only then takes the device (the guard lives in the caller's frame, declared before the scene,
// and hands the caller's device back on return) and uploads them.
int upload_scene(gcsadmm_scene_s &s, std::optional<DeviceGuard> &guard, int n, int P, const int *poly_ptr, const double *A, const double *b,
                 int device)
{
    if (n < 1 || n > 8) { g_err = "polytope LPs are instantiated for n = 1..8"; return GCSADMM_ERR_UNSUPPORTED; }
    if (P < 0 || !poly_ptr || (P > 0 && (!A || !b))) { g_err = "null polytope array"; return GCSADMM_ERR_BAD_ARG; }
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) { g_err = "no HIP device"; return GCSADMM_ERR_NO_DEVICE; }
    if (device < 0 || device >= ndev) { g_err = "device ordinal out of range"; return GCSADMM_ERR_BAD_ARG; }
    if (poly_ptr[0] != 0) { g_err = "poly_ptr[0] != 0"; return GCSADMM_ERR_BAD_ARG; }
    for (int p = 0; p < P; ++p) {
        const int m = poly_ptr[p + 1] - poly_ptr[p];
        if (m < 1) { g_err = "polytope without rows"; return GCSADMM_ERR_BAD_ARG; }
        s.maxm = std::max(s.maxm, m);
    }
    const size_t rows = (size_t)poly_ptr[P];
    std::vector<double> nrm(rows);
    for (size_t r = 0; r < rows; ++r) {
        double sq = 0;
        for (int k = 0; k < n; ++k) sq += A[r * n + k] * A[r * n + k];
        if (!(sq > 0.0)) { g_err = "zero facet normal"; return GCSADMM_ERR_BAD_ARG; }
        nrm[r] = std::sqrt(sq);
    }
    guard.emplace(device);
    if (int rc = guard_status(*guard)) return rc;
    LPCHK(s.ptr.upload(poly_ptr, (size_t)P + 1));
    if (rows > 0) {      // (upload copies one element even for a count of 0)
        LPCHK(s.A.upload(A, rows * n)); LPCHK(s.b.upload(b, rows)); LPCHK(s.nrm.upload(nrm.data(), rows));
    }
    s.n = n; s.P = P; s.device = device;
    s.S = Polys{n, P, s.ptr.get(), s.A.get(), s.b.get(), s.nrm.get()};
    return GCSADMM_OK;
}

// The buffers of the stages are allocated here and nowhere else: gcsadmm_scene_create takes a resident scene's, and
// gcsadmm_scene_candidate_pairs the pair list's once it knows T; a batch call takes those of its one stage.
enum : unsigned {
    BUF_CEN = 1,            // the centres: written by the centre stage, read by the other two
    BUF_CENTRE_LP = 2, BUF_BOXES = 4, BUF_PAIRS = 8,
    BUF_RESIDENT = 16       // the sweep's arrays and the counts of decisions: what only a resident scene has
};
int alloc_buffers(gcsadmm_scene_s *s, unsigned which, size_t T = 0)
{
    const size_t P = (size_t)s->P, n = (size_t)s->n;
    hipError_t e = hipSuccess;
    auto take = [&](unsigned group, auto &buf, size_t count) {
        if (!(which & group) || e != hipSuccess) return;
        buf.reset();      // (before the new one is taken: a pair list is replaced, not held twice)
        e = buf.alloc(count);
    };
    take(BUF_CEN, s->cen, P * n);
    take(BUF_CENTRE_LP, s->w, P * (n + 1)); take(BUF_CENTRE_LP, s->rad, P); take(BUF_CENTRE_LP, s->st_c, P);
    take(BUF_BOXES, s->lo, P * n); take(BUF_BOXES, s->hi, P * n); take(BUF_BOXES, s->st_b, P * 2 * n);
    take(BUF_RESIDENT, s->lo0, P); take(BUF_RESIDENT, s->order, P); take(BUF_RESIDENT, s->slo, P * n); take(BUF_RESIDENT, s->shi, P * n);
    take(BUF_RESIDENT, s->count, P); take(BUF_RESIDENT, s->offset, P); take(BUF_RESIDENT, s->counts, 2);
    take(BUF_PAIRS, s->pa, T); take(BUF_PAIRS, s->pb, T); take(BUF_PAIRS, s->flag, T); take(BUF_PAIRS, s->st_o, T);
    if (e != hipSuccess) { g_err = std::string("hipMalloc: ") + hipGetErrorString(e); return GCSADMM_ERR_HIP; }
    return GCSADMM_OK;
}

// all of a buffer to the host; dst == nullptr: the caller does not want it
template <class T> hipError_t download(T *dst, const DevBuf<T> &src)
{
    return dst ? hipMemcpy(dst, src.get(), sizeof(T) * src.size(), hipMemcpyDeviceToHost) : hipSuccess;
}

// ---- the launches ----
template <int N>
int launch_ball(const gcsadmm_scene_s &s, long count, const int *d_pa, const int *d_pb, const double *d_x0, int rows_max, double tol, int early,
                double *d_w, unsigned char *d_flag, int *d_status)
{
    const size_t lds = lds_bytes(rows_max);
    if (lds > LDS_MAX_BYTES) { g_err = "too many facet rows per LP for LDS"; return GCSADMM_ERR_UNSUPPORTED; }
    LPCHK(hipFuncSetAttribute((const void *)ball_kernel<N>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    if (count > 0)
        hipLaunchKernelGGL(ball_kernel<N>, dim3((unsigned)((count + WAVE - 1) / WAVE)), dim3(WAVE), lds, 0, s.S, (int)count, d_pa, d_pb,
                           d_x0, rows_max, tol, early, d_w, d_flag, d_status);
    LPCHK(hipGetLastError());
    return GCSADMM_OK;
}

template <int N>
int launch_bounds(const gcsadmm_scene_s &s, int first, int polys, const double *d_centers, double *d_lo, double *d_hi, int *d_status)
{
    const int rows_max = bounds_rows(s.maxm, N);
    const size_t lds = lds_bytes(rows_max);
    if (lds > LDS_MAX_BYTES) { g_err = "too many facet rows per LP for LDS"; return GCSADMM_ERR_UNSUPPORTED; }
    LPCHK(hipFuncSetAttribute((const void *)bounds_kernel<N>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    const long count = (long)polys * 2 * N;
    if (count > 0)
        hipLaunchKernelGGL(bounds_kernel<N>, dim3((unsigned)((count + WAVE - 1) / WAVE)), dim3(WAVE), lds, 0, s.S, first, polys, d_centers, rows_max, d_lo,
                           d_hi, d_status);
    LPCHK(hipGetLastError());
    return GCSADMM_OK;
}

template <int N>
int launch_sweep(gcsadmm_scene_s *s, bool fill, double pad)
{
    const SortedBoxes B{s->P, s->slo.get(), s->shi.get(), s->order.get()};
    if (s->P > 0) {
        if (fill)
            hipLaunchKernelGGL((sweep_kernel<N, true>), dim3((unsigned)s->P), dim3(SWEEP_WAVE), 0, 0, B, pad, nullptr, s->offset.get(), s->pa.get(),
                               s->pb.get());
        else
            hipLaunchKernelGGL((sweep_kernel<N, false>), dim3((unsigned)s->P), dim3(SWEEP_WAVE), 0, 0, B, pad, s->count.get(), nullptr, nullptr, nullptr);
    }
    LPCHK(hipGetLastError());
    return GCSADMM_OK;
}

template <int N>
int launch_restrict(const gcsadmm_k::RestrictPlan &rp, const RestrictArgs &a)
{
    hipLaunchKernelGGL(path_restrict_kernel<N>, dim3((unsigned)rp.grid), dim3((unsigned)rp.threads), 0, 0, a);
    LPCHK(hipGetLastError());
    return GCSADMM_OK;
}

// room for count elements in a buffer that outlives the call (the query buffers: a call with no more points or hits than an earlier
// one allocates nothing)
template <class T> hipError_t reserve(DevBuf<T> &buf, size_t count)
{
    if (buf && buf.size() >= count) return hipSuccess;
    buf.reset();
    return buf.alloc(count);
}

template <int N>
int launch_locate(const LocateArgs &args, long long num_points, bool fill)
{
    constexpr long long SLAB = 65535;      // grid.y
    for (long long q0 = 0; q0 < num_points; q0 += SLAB) {
        LocateArgs a = args;
        a.first_point = (int)q0;
        const dim3 grid((unsigned)a.chunks, (unsigned)std::min(SLAB, num_points - q0));
        if (fill) hipLaunchKernelGGL((locate_kernel<N, true>), grid, dim3(LOCATE_WAVE), 0, 0, a);
        else hipLaunchKernelGGL((locate_kernel<N, false>), grid, dim3(LOCATE_WAVE), 0, 0, a);
        LPCHK(hipGetLastError());
    }
    return GCSADMM_OK;
}

// ---- the three LP stages, on the scene's buffers: what both families of entry points run ----
// centre LPs of all polytopes into w and st_c, then the centres and radii out of the records
int run_centers(gcsadmm_scene_s *s)
{
    const int rc = for_dim(s->n, [&](auto N) {
        return launch_ball<decltype(N)::value>(*s, s->P, nullptr, nullptr, nullptr, centre_rows(s->maxm), 0.0, 0, s->w.get(), nullptr, s->st_c.get());
    });
    if (rc != GCSADMM_OK) return rc;
    if (s->P > 0) hipLaunchKernelGGL(split_centres_kernel, dim3(blocks_of(s->P)), dim3(TB), 0, 0, s->w.get(), s->n, s->P, s->cen.get(), s->rad.get());
    LPCHK(hipGetLastError());
    return GCSADMM_OK;
}

// the 2n bound LPs of every polytope, started at cen, into lo, hi and st_b: what the LPs left (a failed side is not opened here)
int run_bounds(gcsadmm_scene_s *s)
{
    return for_dim(s->n, [&](auto N) { return launch_bounds<decltype(N)::value>(*s, 0, s->P, s->cen.get(), s->lo.get(), s->hi.get(), s->st_b.get()); });
}

// one LP per pair of pa, pb into flag and st_o; x0: the scene's centres (LP t starts at x0[pa[t]]), or nullptr (least-squares points)
int run_overlaps(gcsadmm_scene_s *s, const double *x0, double tol)
{
    return for_dim(s->n, [&](auto N) {
        return launch_ball<decltype(N)::value>(*s, (long)s->T, s->pa.get(), s->pb.get(), x0, overlap_rows(s->maxm), tol, 1, nullptr, s->flag.get(),
                                               s->st_o.get());
    });
}

// ---- their results to the host (a null pointer: not wanted) ----
int read_centers(gcsadmm_scene_s *s, double *centers, double *radii, int *status)
{
    LPCHK(download(centers, s->cen)); LPCHK(download(radii, s->rad)); LPCHK(download(status, s->st_c));
    return GCSADMM_OK;
}
int read_boxes(gcsadmm_scene_s *s, double *lo, double *hi, int *status)
{
    LPCHK(download(lo, s->lo)); LPCHK(download(hi, s->hi)); LPCHK(download(status, s->st_b));
    return GCSADMM_OK;
}
int read_decisions(gcsadmm_scene_s *s, unsigned char *overlap, int *status)
{
    LPCHK(download(overlap, s->flag)); LPCHK(download(status, s->st_o));
    return GCSADMM_OK;
}

} // namespace

extern "C" {

const char *gcsadmm_polytope_last_error(void) { return g_err.c_str(); }

// ---- batch calls: a scene for the length of the call, with the buffers of one stage; host arrays in, host arrays out ----
int gcsadmm_polytope_centers(int n, int num_polytopes, const int *poly_ptr, const double *poly_A, const double *poly_b,
                             int device, double *centers, double *radii, int *status)
{
    if (!centers) { g_err = "null output"; return GCSADMM_ERR_BAD_ARG; }
    std::optional<DeviceGuard> guard;
    gcsadmm_scene_s s;
    int rc = upload_scene(s, guard, n, num_polytopes, poly_ptr, poly_A, poly_b, device);
    if (rc == GCSADMM_OK) rc = alloc_buffers(&s, BUF_CEN | BUF_CENTRE_LP);
    if (rc == GCSADMM_OK) rc = run_centers(&s);
    if (rc == GCSADMM_OK) rc = read_centers(&s, centers, radii, status);
    return rc;
}

int gcsadmm_polytope_bounds(int n, int num_polytopes, const int *poly_ptr, const double *poly_A, const double *poly_b,
                            const double *centers, int device, double *lo, double *hi, int *status)
{
    if (!centers || !lo || !hi) { g_err = "null centres or output"; return GCSADMM_ERR_BAD_ARG; }
    std::optional<DeviceGuard> guard;
    gcsadmm_scene_s s;
    int rc = upload_scene(s, guard, n, num_polytopes, poly_ptr, poly_A, poly_b, device);
    if (rc == GCSADMM_OK) rc = alloc_buffers(&s, BUF_CEN | BUF_BOXES);
    if (rc != GCSADMM_OK) return rc;
    LPCHK(hipMemcpy(s.cen.get(), centers, sizeof(double) * s.cen.size(), hipMemcpyHostToDevice));
    rc = run_bounds(&s);
    if (rc == GCSADMM_OK) rc = read_boxes(&s, lo, hi, status);      // as the LPs left them: opening a failed side is the caller's
    return rc;
}

int gcsadmm_polytope_overlaps(int n, int num_polytopes, const int *poly_ptr, const double *poly_A, const double *poly_b,
                              const double *centers, long num_pairs, const int *pair_a, const int *pair_b, double tol,
                              int device, unsigned char *overlap, int *status)
{
    if (num_pairs < 0 || (num_pairs > 0 && (!pair_a || !pair_b || !overlap))) { g_err = "null pair list or output"; return GCSADMM_ERR_BAD_ARG; }
    for (long t = 0; t < num_pairs; ++t)
        if (pair_a[t] < 0 || pair_a[t] >= num_polytopes || pair_b[t] < 0 || pair_b[t] >= num_polytopes) {
            g_err = "pair index out of range"; return GCSADMM_ERR_BAD_ARG;
        }
    std::optional<DeviceGuard> guard;
    gcsadmm_scene_s s;
    int rc = upload_scene(s, guard, n, num_polytopes, poly_ptr, poly_A, poly_b, device);
    if (rc == GCSADMM_OK) rc = alloc_buffers(&s, (centers ? BUF_CEN : 0u) | BUF_PAIRS, (size_t)num_pairs);
    if (rc != GCSADMM_OK) return rc;
    s.T = num_pairs;
    LPCHK(hipMemcpy(s.pa.get(), pair_a, sizeof(int) * s.pa.size(), hipMemcpyHostToDevice));
    LPCHK(hipMemcpy(s.pb.get(), pair_b, sizeof(int) * s.pb.size(), hipMemcpyHostToDevice));
    if (centers) LPCHK(hipMemcpy(s.cen.get(), centers, sizeof(double) * s.cen.size(), hipMemcpyHostToDevice));
    rc = run_overlaps(&s, s.cen.get(), tol);      // (no centres: no buffer, every LP starts from its least-squares point)
    if (rc == GCSADMM_OK) rc = read_decisions(&s, overlap, status);
    return rc;
}

// ---- the resident scene: precondition, stage, what only it does, results, synchronise, flag ----
int gcsadmm_scene_create(int n, int num_polytopes, const int *poly_ptr, const double *poly_A, const double *poly_b, int device,
                         gcsadmm_scene *out)
{
    if (!out) { g_err = "null output"; return GCSADMM_ERR_BAD_ARG; }
    *out = nullptr;
    std::optional<DeviceGuard> guard;
    gcsadmm_scene_s *s = new (std::nothrow) gcsadmm_scene_s;
    if (!s) { g_err = "out of host memory"; return GCSADMM_ERR_NO_MEMORY; }
    int rc;
    try {
        rc = upload_scene(*s, guard, n, num_polytopes, poly_ptr, poly_A, poly_b, device);
        if (rc == GCSADMM_OK) s->h_ptr.assign(poly_ptr, poly_ptr + num_polytopes + 1);
    } catch (const std::bad_alloc &) {
        g_err = "out of host memory"; rc = GCSADMM_ERR_NO_MEMORY;
    }
    if (rc == GCSADMM_OK) rc = alloc_buffers(s, BUF_CEN | BUF_CENTRE_LP | BUF_BOXES | BUF_RESIDENT);
    if (rc != GCSADMM_OK) { delete s; return rc; }
    *out = s;
    return GCSADMM_OK;
}

void gcsadmm_scene_destroy(gcsadmm_scene s)
{
    if (!s) return;
    DeviceGuard device_guard_(s->device);
    delete s;
}

int gcsadmm_scene_centers(gcsadmm_scene s, double *centers, double *radii, int *status)
{
    USE_SCENE(s);
    s->have_centers = false;
    int rc = run_centers(s);
    if (rc == GCSADMM_OK) rc = read_centers(s, centers, radii, status);
    if (rc != GCSADMM_OK) return rc;
    LPCHK(hipStreamSynchronize(nullptr));
    s->have_centers = true;
    return GCSADMM_OK;
}

int gcsadmm_scene_bounds(gcsadmm_scene s, double *lo, double *hi, int *status)
{
    USE_SCENE(s);
    if (!s->have_centers) { g_err = "no resident centres: call gcsadmm_scene_centers first"; return GCSADMM_ERR_BAD_ARG; }
    s->have_boxes = s->have_pairs = s->have_overlaps = false;
    int rc = run_bounds(s);
    if (rc != GCSADMM_OK) return rc;
    const long sides = (long)s->P * s->n * 2;
    if (sides > 0) hipLaunchKernelGGL(open_failed_sides_kernel, dim3(blocks_of(sides)), dim3(TB), 0, 0, s->st_b.get(), s->n, s->P, s->lo.get(), s->hi.get());
    LPCHK(hipGetLastError());
    if ((rc = read_boxes(s, lo, hi, status)) != GCSADMM_OK) return rc;
    LPCHK(hipStreamSynchronize(nullptr));
    s->have_boxes = true;
    return GCSADMM_OK;
}

int gcsadmm_scene_set_boxes(gcsadmm_scene s, const double *lo, const double *hi)
{
    USE_SCENE(s);
    const size_t cells = (size_t)s->P * s->n;
    if (cells > 0 && (!lo || !hi)) { g_err = "null boxes"; return GCSADMM_ERR_BAD_ARG; }
    for (size_t i = 0; i < cells; ++i)
        if (!(lo[i] <= hi[i])) { g_err = "box with a NaN or with lo > hi"; return GCSADMM_ERR_BAD_ARG; }
    s->have_boxes = s->have_pairs = s->have_overlaps = false;
    LPCHK(hipMemcpy(s->lo.get(), lo, sizeof(double) * cells, hipMemcpyHostToDevice));
    LPCHK(hipMemcpy(s->hi.get(), hi, sizeof(double) * cells, hipMemcpyHostToDevice));
    s->have_boxes = true;
    return GCSADMM_OK;
}

static int candidate_pairs(gcsadmm_scene s, double pad, int64_t *num_pairs)
{
    USE_SCENE(s);
    if (!s->have_boxes) { g_err = "no resident boxes: call gcsadmm_scene_bounds or gcsadmm_scene_set_boxes first"; return GCSADMM_ERR_BAD_ARG; }
    if (!(pad == pad)) { g_err = "pad is NaN"; return GCSADMM_ERR_BAD_ARG; }
    const int n = s->n, P = s->P;
    s->have_pairs = s->have_overlaps = s->have_graph = false;
    s->T = 0;
    // sort on the host (P log P on P doubles; a device radix sort would order -0.0 before +0.0 and change the order of ties)
    std::vector<double> lo0((size_t)P);
    std::vector<int> order((size_t)P), count((size_t)P);
    std::vector<long long> offset((size_t)P);
    if (P > 0) hipLaunchKernelGGL(first_lower_bounds_kernel, dim3(blocks_of(P)), dim3(TB), 0, 0, s->lo.get(), n, P, s->lo0.get());
    LPCHK(hipGetLastError());
    LPCHK(download(lo0.data(), s->lo0));
    for (int p = 0; p < P; ++p)      // a NaN has no place in the order (set_boxes refuses one; a bounds LP reports none with a status >= 0)
        if (!(lo0[p] == lo0[p])) { g_err = "resident box with a NaN lower bound"; return GCSADMM_ERR_BAD_ARG; }
    sweep_order(lo0.data(), P, order.data());
    LPCHK(hipMemcpy(s->order.get(), order.data(), sizeof(int) * (size_t)P, hipMemcpyHostToDevice));
    if (P > 0)
        hipLaunchKernelGGL(sweep_gather_kernel, dim3(blocks_of(P)), dim3(TB), 0, 0, s->lo.get(), s->hi.get(), s->order.get(), n, P, s->slo.get(), s->shi.get());
    LPCHK(hipGetLastError());
    int rc = for_dim(n, [&](auto N) { return launch_sweep<decltype(N)::value>(s, false, pad); });
    if (rc != GCSADMM_OK) return rc;
    LPCHK(download(count.data(), s->count));
    long long total = 0;
    if (!sweep_scan(count.data(), P, offset.data(), &total)) {      // before anything is allocated
        g_err = "more than 2^31 - 1 candidate pairs"; return GCSADMM_ERR_UNSUPPORTED;
    }
    if ((rc = alloc_buffers(s, BUF_PAIRS, (size_t)total)) != GCSADMM_OK) return rc;
    LPCHK(hipMemcpy(s->offset.get(), offset.data(), sizeof(long long) * (size_t)P, hipMemcpyHostToDevice));
    if (total > 0) {
        rc = for_dim(n, [&](auto N) { return launch_sweep<decltype(N)::value>(s, true, pad); });
        if (rc != GCSADMM_OK) return rc;
    }
    LPCHK(hipStreamSynchronize(nullptr));
    s->T = total;
    s->have_pairs = true;
    if (num_pairs) *num_pairs = total;
    return GCSADMM_OK;
}

int gcsadmm_scene_candidate_pairs(gcsadmm_scene s, double pad, int64_t *num_pairs)
{
    try {
        return candidate_pairs(s, pad, num_pairs);
    } catch (const std::bad_alloc &) {      // the host arrays of the sort and the scan
        g_err = "out of host memory"; return GCSADMM_ERR_NO_MEMORY;
    }
}

int gcsadmm_scene_overlaps(gcsadmm_scene s, double tol, int64_t *num_overlapping, int64_t *num_undecided)
{
    USE_SCENE(s);
    if (!s->have_pairs) { g_err = "no resident pairs: call gcsadmm_scene_candidate_pairs first"; return GCSADMM_ERR_BAD_ARG; }
    if (!s->have_centers) { g_err = "no resident centres: call gcsadmm_scene_centers first"; return GCSADMM_ERR_BAD_ARG; }
    s->have_overlaps = s->have_graph = false;
    const int rc = run_overlaps(s, s->cen.get(), tol);
    if (rc != GCSADMM_OK) return rc;
    if (num_overlapping || num_undecided) {      // counted where the flags are: two numbers come back, the arrays stay for read_pairs
        unsigned long long counts[2] = {0, 0};
        LPCHK(hipMemcpy(s->counts.get(), counts, sizeof(counts), hipMemcpyHostToDevice));
        if (s->T > 0)
            hipLaunchKernelGGL(count_decisions_kernel, dim3(blocks_of((long)s->T)), dim3(TB), 0, 0, s->flag.get(), s->st_o.get(), (long)s->T, s->counts.get());
        LPCHK(hipGetLastError());
        LPCHK(download(counts, s->counts));
        if (num_overlapping) *num_overlapping = (int64_t)counts[0];
        if (num_undecided) *num_undecided = (int64_t)counts[1];
    }
    LPCHK(hipStreamSynchronize(nullptr));
    s->have_overlaps = true;
    return GCSADMM_OK;
}

int gcsadmm_scene_read_pairs(gcsadmm_scene s, int *pair_a, int *pair_b, unsigned char *overlap, int *status)
{
    USE_SCENE(s);
    if (!s->have_pairs) { g_err = "no resident pairs: call gcsadmm_scene_candidate_pairs first"; return GCSADMM_ERR_BAD_ARG; }
    if ((overlap || status) && !s->have_overlaps) { g_err = "the resident pairs are not decided: call gcsadmm_scene_overlaps first"; return GCSADMM_ERR_BAD_ARG; }
    LPCHK(download(pair_a, s->pa)); LPCHK(download(pair_b, s->pb));
    return read_decisions(s, overlap, status);
}

static int restrict_paths(gcsadmm_scene s, int num_paths, const int *path_ptr, const int *path_poly, const double *start, double tol,
                          int max_iter, double *points, double *cost, int *iterations, int *status)
{
    USE_SCENE(s);
    gcsadmm_k::RestrictPlan rp;
    if (int rc = gcsadmm_k::make_restrict_plan(s->n, s->P, s->h_ptr.data(), num_paths, path_ptr, path_poly, rp, g_err)) return rc;
    if (!(tol > 0.0) || max_iter < 0) { g_err = "tol must be positive and max_iter non-negative"; return GCSADMM_ERR_BAD_ARG; }
    if (num_paths == 0) return GCSADMM_OK;
    if (!start) { g_err = "null start"; return GCSADMM_ERR_BAD_ARG; }
    const size_t coords = (size_t)rp.total_points * s->n;
    DevBuf<int> d_path_ptr, d_path_poly, d_prefix, d_iterations, d_status;
    DevBuf<long long> d_ws_off;
    DevBuf<double> d_ws, d_start, d_points, d_cost;
    LPCHK(d_path_ptr.upload(path_ptr, (size_t)num_paths + 1));
    LPCHK(d_path_poly.upload(path_poly, (size_t)rp.total_regions));
    LPCHK(d_prefix.upload(rp.row_prefix.data(), rp.row_prefix.size()));
    LPCHK(d_ws_off.upload(rp.ws_off.data(), rp.ws_off.size()));
    LPCHK(d_start.upload(start, coords));
    LPCHK(d_ws.alloc((size_t)rp.ws_doubles));
    LPCHK(d_points.alloc(coords)); LPCHK(d_cost.alloc((size_t)num_paths));
    LPCHK(d_iterations.alloc((size_t)num_paths)); LPCHK(d_status.alloc((size_t)num_paths));
    const RestrictArgs a{s->ptr.get(), s->A.get(), s->b.get(), d_path_ptr.get(), d_path_poly.get(), d_prefix.get(), d_ws_off.get(), d_ws.get(),
                         d_start.get(), d_points.get(), d_cost.get(), d_iterations.get(), d_status.get(), tol, max_iter, num_paths};
    const int rc = for_dim(s->n, [&](auto N) { return launch_restrict<decltype(N)::value>(rp, a); });
    if (rc != GCSADMM_OK) return rc;
    LPCHK(download(points, d_points)); LPCHK(download(cost, d_cost)); LPCHK(download(iterations, d_iterations)); LPCHK(download(status, d_status));
    LPCHK(hipStreamSynchronize(nullptr));
    return GCSADMM_OK;
}

int gcsadmm_scene_restrict_paths(gcsadmm_scene s, int num_paths, const int *path_ptr, const int *path_poly, const double *start, double tol,
                                 int max_iter, double *points, double *cost, int *iterations, int *status)
{
    try {
        return restrict_paths(s, num_paths, path_ptr, path_poly, start, tol, max_iter, points, cost, iterations, status);
    } catch (const std::bad_alloc &) {      // the plan's host arrays
        g_err = "out of host memory"; return GCSADMM_ERR_NO_MEMORY;
    }
}

static int locate_points(gcsadmm_scene s, int num_points, const double *points, double eps, double tol, int64_t *num_hits)
{
    USE_SCENE(s);
    if (num_points < 0 || (num_points > 0 && !points)) { g_err = "negative number of points or null points"; return GCSADMM_ERR_BAD_ARG; }
    if (!(eps >= 0.0) || !(tol >= 0.0) || std::isinf(eps) || std::isinf(tol)) { g_err = "eps and tol must be finite and non-negative"; return GCSADMM_ERR_BAD_ARG; }
    const size_t coords = (size_t)num_points * s->n;
    for (size_t i = 0; i < coords; ++i)
        if (!std::isfinite(points[i])) { g_err = "point with a NaN or an inf coordinate"; return GCSADMM_ERR_BAD_ARG; }
    s->have_hits = false;
    const long long Q = num_points, chunks = locate_chunks(s->P);
    const size_t cells = (size_t)(Q * chunks);
    std::vector<int> count(cells);
    std::vector<long long> offset(cells);
    std::vector<int64_t> hit_ptr((size_t)Q + 1, 0);
    LocateArgs a{};
    a.R = LocateRegions{s->P, s->ptr.get(), s->A.get(), s->b.get()};
    a.margin = eps + 2.0 * tol;
    a.chunks = chunks;
    long long total = 0;
    if (cells > 0) {
        LPCHK(reserve(s->q_points, coords)); LPCHK(reserve(s->q_count, cells));
        LPCHK(hipMemcpy(s->q_points.get(), points, sizeof(double) * coords, hipMemcpyHostToDevice));
        a.points = s->q_points.get(); a.count = s->q_count.get();
        int rc = for_dim(s->n, [&](auto N) { return launch_locate<decltype(N)::value>(a, Q, false); });
        if (rc != GCSADMM_OK) return rc;
        LPCHK(hipMemcpy(count.data(), s->q_count.get(), sizeof(int) * cells, hipMemcpyDeviceToHost));
        if (!locate_scan(count.data(), Q, chunks, offset.data(), hit_ptr.data())) {      // before the list is allocated
            g_err = "more than 2^31 - 1 hits"; return GCSADMM_ERR_UNSUPPORTED;
        }
        total = hit_ptr[(size_t)Q];
    }
    if (total > 0) {
        LPCHK(reserve(s->hit_region, (size_t)total)); LPCHK(reserve(s->hit_class, (size_t)total)); LPCHK(reserve(s->q_offset, cells));
        LPCHK(hipMemcpy(s->q_offset.get(), offset.data(), sizeof(long long) * cells, hipMemcpyHostToDevice));
        a.offset = s->q_offset.get(); a.limit = total;
        a.hit_region = s->hit_region.get(); a.hit_class = s->hit_class.get();
        const int rc = for_dim(s->n, [&](auto N) { return launch_locate<decltype(N)::value>(a, Q, true); });
        if (rc != GCSADMM_OK) return rc;
    }
    LPCHK(hipStreamSynchronize(nullptr));
    s->hit_ptr.swap(hit_ptr);
    s->have_hits = true;
    if (num_hits) *num_hits = total;
    return GCSADMM_OK;
}

int gcsadmm_scene_locate_points(gcsadmm_scene s, int num_points, const double *points, double eps, double tol, int64_t *num_hits)
{
    try {
        return locate_points(s, num_points, points, eps, tol, num_hits);
    } catch (const std::bad_alloc &) {      // the host arrays of the scan
        g_err = "out of host memory"; return GCSADMM_ERR_NO_MEMORY;
    }
}

int gcsadmm_scene_read_hits(gcsadmm_scene s, int64_t *hit_ptr, int *hit_region, unsigned char *hit_class)
{
    USE_SCENE(s);
    if (!s->have_hits) { g_err = "no resident hit list: call gcsadmm_scene_locate_points first"; return GCSADMM_ERR_BAD_ARG; }
    if (hit_ptr) std::copy(s->hit_ptr.begin(), s->hit_ptr.end(), hit_ptr);
    const size_t total = (size_t)s->hit_ptr.back();      // (the buffers may be longer: they are kept from call to call)
    if (hit_region && total) LPCHK(hipMemcpy(hit_region, s->hit_region.get(), sizeof(int) * total, hipMemcpyDeviceToHost));
    if (hit_class && total) LPCHK(hipMemcpy(hit_class, s->hit_class.get(), total, hipMemcpyDeviceToHost));
    return GCSADMM_OK;
}

} // extern "C"

// ---- edits of a decided scene: everything is built in a scene of its own beside the resident one, and takes its place at the end ----
namespace {

// a new buffer of `count` elements with the first `old` ones of src (device) and `fresh` host elements behind them
template <class T> hipError_t grown(DevBuf<T> &dst, const DevBuf<T> &src, size_t old, const T *fresh, size_t count)
{
    hipError_t e = dst.alloc(count);
    if (e == hipSuccess && old > 0) e = hipMemcpy(dst.get(), src.get(), sizeof(T) * old, hipMemcpyDeviceToDevice);
    if (e == hipSuccess && fresh && count > old) e = hipMemcpy(dst.get() + old, fresh, sizeof(T) * (count - old), hipMemcpyHostToDevice);
    return e;
}
template <class T> hipError_t put(DevBuf<T> &dst, const T *src, size_t count) { return grown(dst, dst, 0, src, count); }
// the first `count` elements of src into a buffer that is already there
template <class T> hipError_t carry(DevBuf<T> &dst, const DevBuf<T> &src, size_t count)
{
    return count > 0 ? hipMemcpy(dst.get(), src.get(), sizeof(T) * count, hipMemcpyDeviceToDevice) : hipSuccess;
}
template <class T> hipError_t fetch(T *dst, const T *src, size_t count)
{
    return count > 0 ? hipMemcpy(dst, src, sizeof(T) * count, hipMemcpyDeviceToHost) : hipSuccess;
}

template <int N> int launch_cross(const CrossSide &side, int sweepers, double pad, bool fill)
{
    constexpr int SLAB = 65535;      // grid.y
    if (side.chunks <= 0) return GCSADMM_OK;
    for (int k0 = 0; k0 < sweepers; k0 += SLAB) {
        CrossSide c = side;
        c.first = k0;
        const dim3 grid((unsigned)c.chunks, (unsigned)std::min(SLAB, sweepers - k0));
        if (fill) hipLaunchKernelGGL((cross_kernel<N, true>), grid, dim3(SWEEP_WAVE), 0, 0, c, pad);
        else hipLaunchKernelGGL((cross_kernel<N, false>), grid, dim3(SWEEP_WAVE), 0, 0, c, pad);
        LPCHK(hipGetLastError());
    }
    return GCSADMM_OK;
}

// the edited scene takes the place of the resident one (nothing here can fail)
void commit_regions(gcsadmm_scene_s *s, gcsadmm_scene_s &nx, std::vector<int> &h_ptr)
{
    std::swap(s->ptr, nx.ptr); std::swap(s->A, nx.A); std::swap(s->b, nx.b); std::swap(s->nrm, nx.nrm);
    std::swap(s->w, nx.w); std::swap(s->cen, nx.cen); std::swap(s->rad, nx.rad); std::swap(s->st_c, nx.st_c);
    std::swap(s->lo, nx.lo); std::swap(s->hi, nx.hi); std::swap(s->st_b, nx.st_b);
    std::swap(s->lo0, nx.lo0); std::swap(s->slo, nx.slo); std::swap(s->shi, nx.shi);
    std::swap(s->order, nx.order); std::swap(s->count, nx.count); std::swap(s->offset, nx.offset);
    s->h_ptr.swap(h_ptr);
    s->P = nx.P; s->maxm = nx.maxm;
    s->S = Polys{s->n, s->P, s->ptr.get(), s->A.get(), s->b.get(), s->nrm.get()};
    s->have_hits = s->have_graph = false;
}
void commit_pairs(gcsadmm_scene_s *s, gcsadmm_scene_s &nx, long long T)
{
    std::swap(s->pa, nx.pa); std::swap(s->pb, nx.pb); std::swap(s->flag, nx.flag); std::swap(s->st_o, nx.st_o);
    s->T = T;
    s->have_graph = false;
}

} // namespace

extern "C" {

static int add_regions(gcsadmm_scene s, int K, const int *poly_ptr, const double *A, const double *b, double pad, double tol, double *centers,
                       double *radii, int *center_status, int64_t *num_new_pairs, int64_t *num_overlapping, int64_t *num_undecided)
{
    USE_SCENE(s);
    if (!s->have_centers) { g_err = "no resident centres: call gcsadmm_scene_centers first"; return GCSADMM_ERR_BAD_ARG; }
    if (!s->have_boxes) { g_err = "no resident boxes: call gcsadmm_scene_bounds or gcsadmm_scene_set_boxes first"; return GCSADMM_ERR_BAD_ARG; }
    if (!s->have_pairs) { g_err = "no resident pairs: call gcsadmm_scene_candidate_pairs first"; return GCSADMM_ERR_BAD_ARG; }
    if (!s->have_overlaps) { g_err = "the resident pairs are not decided: call gcsadmm_scene_overlaps first"; return GCSADMM_ERR_BAD_ARG; }
    if (K < 0 || !poly_ptr || (K > 0 && (!A || !b))) { g_err = "negative number of regions or null polytope array"; return GCSADMM_ERR_BAD_ARG; }
    if (!(pad == pad)) { g_err = "pad is NaN"; return GCSADMM_ERR_BAD_ARG; }
    if (poly_ptr[0] != 0) { g_err = "poly_ptr[0] != 0"; return GCSADMM_ERR_BAD_ARG; }
    const int n = s->n, P = s->P;
    const size_t un = (size_t)n, uP = (size_t)P, uK = (size_t)K;
    gcsadmm_scene_s nx;
    nx.n = n; nx.device = s->device; nx.maxm = s->maxm;
    for (int p = 0; p < K; ++p) {
        const int m = poly_ptr[p + 1] - poly_ptr[p];
        if (m < 1) { g_err = "polytope without rows"; return GCSADMM_ERR_BAD_ARG; }
        nx.maxm = std::max(nx.maxm, m);
    }
    const size_t old_rows = (size_t)s->h_ptr[uP], new_rows = (size_t)poly_ptr[K];
    if ((long long)P + K > INT32_MAX || (long long)old_rows + (long long)new_rows > INT32_MAX) {
        g_err = "more than 2^31 - 1 regions or rows"; return GCSADMM_ERR_UNSUPPORTED;
    }
    std::vector<double> nrm(new_rows);
    for (size_t r = 0; r < new_rows; ++r) {
        double sq = 0;
        for (int k = 0; k < n; ++k) sq += A[r * un + k] * A[r * un + k];
        if (!(sq > 0.0)) { g_err = "zero facet normal"; return GCSADMM_ERR_BAD_ARG; }
        nrm[r] = std::sqrt(sq);
    }
    if (num_new_pairs) *num_new_pairs = 0;
    if (num_overlapping) *num_overlapping = 0;
    if (num_undecided) *num_undecided = 0;
    if (K == 0) return GCSADMM_OK;
    nx.P = P + K;
    std::vector<int> h_ptr(s->h_ptr), appended(uK);
    for (int p = 1; p <= K; ++p) h_ptr.push_back((int)old_rows + poly_ptr[p]);
    for (int p = 0; p < K; ++p) appended[p] = P + p;

    // the polytopes and the results of the resident regions
    LPCHK(put(nx.ptr, h_ptr.data(), h_ptr.size()));
    LPCHK(grown(nx.A, s->A, old_rows * un, A, (old_rows + new_rows) * un));
    LPCHK(grown(nx.b, s->b, old_rows, b, old_rows + new_rows));
    LPCHK(grown(nx.nrm, s->nrm, old_rows, nrm.data(), old_rows + new_rows));
    nx.S = Polys{n, nx.P, nx.ptr.get(), nx.A.get(), nx.b.get(), nx.nrm.get()};
    int rc = alloc_buffers(&nx, BUF_CEN | BUF_CENTRE_LP | BUF_BOXES | BUF_RESIDENT);
    if (rc != GCSADMM_OK) return rc;
    LPCHK(carry(nx.w, s->w, uP * (un + 1))); LPCHK(carry(nx.cen, s->cen, uP * un)); LPCHK(carry(nx.rad, s->rad, uP)); LPCHK(carry(nx.st_c, s->st_c, uP));
    LPCHK(carry(nx.lo, s->lo, uP * un)); LPCHK(carry(nx.hi, s->hi, uP * un)); LPCHK(carry(nx.st_b, s->st_b, uP * 2 * un));

    // centre LPs of the new regions; a region without a centre or without interior ends the call, the resident scene untouched
    DevBuf<int> d_appended;
    LPCHK(put(d_appended, appended.data(), uK));
    rc = for_dim(n, [&](auto N) {
        return launch_ball<decltype(N)::value>(nx, K, d_appended.get(), nullptr, nullptr, centre_rows(nx.maxm), 0.0, 0, nx.w.get() + uP * (un + 1), nullptr,
                                               nx.st_c.get() + uP);
    });
    if (rc != GCSADMM_OK) return rc;
    hipLaunchKernelGGL(split_centres_kernel, dim3(blocks_of(K)), dim3(TB), 0, 0, nx.w.get() + uP * (un + 1), n, K, nx.cen.get() + uP * un, nx.rad.get() + uP);
    LPCHK(hipGetLastError());
    std::vector<double> rad(uK);
    std::vector<int> st_c(uK);
    LPCHK(fetch(rad.data(), nx.rad.get() + uP, uK)); LPCHK(fetch(st_c.data(), nx.st_c.get() + uP, uK));
    if (centers) LPCHK(fetch(centers, nx.cen.get() + uP * un, uK * un));
    if (radii) std::copy(rad.begin(), rad.end(), radii);
    if (center_status) std::copy(st_c.begin(), st_c.end(), center_status);
    for (int p = 0; p < K; ++p) {
        if (st_c[p] < 0) { g_err = "centre LP did not converge for new region " + std::to_string(p); return GCSADMM_ERR_BAD_ARG; }
        if (!(rad[p] > 0.0)) { g_err = "new region " + std::to_string(p) + " has no interior"; return GCSADMM_ERR_BAD_ARG; }
    }

    // their boxes, failed sides opened
    rc = for_dim(n, [&](auto N) {
        return launch_bounds<decltype(N)::value>(nx, P, K, nx.cen.get(), nx.lo.get(), nx.hi.get(), nx.st_b.get() + uP * 2 * un);
    });
    if (rc != GCSADMM_OK) return rc;
    hipLaunchKernelGGL(open_failed_sides_kernel, dim3(blocks_of((long)K * 2 * n)), dim3(TB), 0, 0, nx.st_b.get() + uP * 2 * un, n, K, nx.lo.get() + uP * un,
                       nx.hi.get() + uP * un);
    LPCHK(hipGetLastError());

    // sweep order of the new boxes (sorted on the host, as the resident ones were), ranks of all boxes, the merged sweep arrays
    std::vector<double> lo_new(uK * un), alo0(uK);
    LPCHK(fetch(lo_new.data(), nx.lo.get() + uP * un, uK * un));
    for (int p = 0; p < K; ++p) {
        alo0[p] = lo_new[(size_t)p * un];
        if (!(alo0[p] == alo0[p])) { g_err = "new box with a NaN lower bound"; return GCSADMM_ERR_BAD_ARG; }
    }
    std::vector<int> aorder(uK);
    sweep_order(alo0.data(), K, aorder.data());
    DevBuf<int> d_aorder, d_arank, d_inv, d_oldpos;
    DevBuf<double> aslo, ashi;
    LPCHK(put(d_aorder, aorder.data(), uK));
    LPCHK(d_arank.alloc(uK)); LPCHK(d_inv.alloc(uP + uK)); LPCHK(d_oldpos.alloc(uP + uK));
    LPCHK(aslo.alloc(uK * un)); LPCHK(ashi.alloc(uK * un));
    hipLaunchKernelGGL(sweep_gather_kernel, dim3(blocks_of(K)), dim3(TB), 0, 0, nx.lo.get() + uP * un, nx.hi.get() + uP * un, d_aorder.get(), n, K, aslo.get(),
                       ashi.get());
    const EditRanks ranks{P, K, s->slo.get(), aslo.get(), s->order.get(), d_aorder.get(), d_arank.get(), nx.order.get(), d_inv.get(),
                          d_oldpos.get()};
    hipLaunchKernelGGL(edit_rank_kernel, dim3(blocks_of(nx.P)), dim3(TB), 0, 0, ranks);
    hipLaunchKernelGGL(sweep_gather_kernel, dim3(blocks_of(nx.P)), dim3(TB), 0, 0, nx.lo.get(), nx.hi.get(), nx.order.get(), n, nx.P, nx.slo.get(), nx.shi.get());
    LPCHK(hipGetLastError());

    // cross sweep, count pass: the new boxes over all boxes behind them (F), the resident boxes over the new boxes behind them (B)
    CrossSide F{}, B{};
    F.S = SortedBoxes{K, aslo.get(), ashi.get(), d_aorder.get()}; F.T = SortedBoxes{nx.P, nx.slo.get(), nx.shi.get(), nx.order.get()};
    F.srank = d_arank.get(); F.chunks = edit_chunks(nx.P); F.cell0 = 0;
    B.S = SortedBoxes{P, s->slo.get(), s->shi.get(), s->order.get()}; B.T = F.S;
    B.trank = d_arank.get(); B.chunks = edit_chunks(K); B.cell0 = (long long)K * F.chunks;
    F.norder = B.norder = nx.order.get();
    const long long cells = B.cell0 + (long long)P * B.chunks;
    if (cells > INT32_MAX) { g_err = "more than 2^31 - 1 cells of the cross sweep: add fewer regions per call"; return GCSADMM_ERR_UNSUPPORTED; }
    DevBuf<int> d_cells;
    LPCHK(d_cells.alloc((size_t)cells));
    F.count = B.count = d_cells.get();
    auto cross = [&](bool fill) {
        int r = for_dim(n, [&](auto N) { return launch_cross<decltype(N)::value>(F, K, pad, fill); });
        if (r == GCSADMM_OK) r = for_dim(n, [&](auto N) { return launch_cross<decltype(N)::value>(B, P, pad, fill); });
        return r;
    };
    if ((rc = cross(false)) != GCSADMM_OK) return rc;
    std::vector<int> cell_count((size_t)cells);
    std::vector<long long> cell_off((size_t)cells + 1);
    LPCHK(fetch(cell_count.data(), d_cells.get(), (size_t)cells));
    if (!edit_scan(cell_count.data(), cells, cell_off.data()) || cell_off[(size_t)cells] + s->T > (long long)INT32_MAX) {      // before anything is allocated
        g_err = "more than 2^31 - 1 candidate pairs"; return GCSADMM_ERR_UNSUPPORTED;
    }
    const long long Tn = cell_off[(size_t)cells], T = s->T + Tn;

    // fill pass, then the LPs of the new pairs, each from the centre of its first region
    DevBuf<long long> d_cell_off;
    DevBuf<int> rank_e, rank_l, npa, npb, nst;
    DevBuf<unsigned char> nflag;
    LPCHK(put(d_cell_off, cell_off.data(), cell_off.size()));
    LPCHK(rank_e.alloc((size_t)Tn)); LPCHK(rank_l.alloc((size_t)Tn)); LPCHK(npa.alloc((size_t)Tn)); LPCHK(npb.alloc((size_t)Tn));
    LPCHK(nst.alloc((size_t)Tn)); LPCHK(nflag.alloc((size_t)Tn));
    F.offset = B.offset = d_cell_off.get(); F.limit = B.limit = Tn;
    F.rank_e = B.rank_e = rank_e.get(); F.rank_l = B.rank_l = rank_l.get(); F.pair_a = B.pair_a = npa.get(); F.pair_b = B.pair_b = npb.get();
    if (Tn > 0 && (rc = cross(true)) != GCSADMM_OK) return rc;
    rc = for_dim(n, [&](auto N) {
        return launch_ball<decltype(N)::value>(nx, (long)Tn, npa.get(), npb.get(), nx.cen.get(), overlap_rows(nx.maxm), tol, 1, nullptr, nflag.get(), nst.get());
    });
    if (rc != GCSADMM_OK) return rc;
    unsigned long long decided[2] = {0, 0};
    LPCHK(hipMemcpy(s->counts.get(), decided, sizeof(decided), hipMemcpyHostToDevice));
    if (Tn > 0)
        hipLaunchKernelGGL(count_decisions_kernel, dim3(blocks_of((long)Tn)), dim3(TB), 0, 0, nflag.get(), nst.get(), (long)Tn, s->counts.get());
    LPCHK(hipGetLastError());
    LPCHK(download(decided, s->counts));

    // merge: counts by rank, scan, every pair to its place
    EditMerge m{};
    m.P = P; m.K = K; m.T_old = s->T; m.T_new = Tn; m.chunks_f = F.chunks; m.chunks_b = B.chunks; m.cell_off = d_cell_off.get();
    m.oldpos = d_oldpos.get(); m.inv = d_inv.get(); m.count_old = s->count.get(); m.offset_old = s->offset.get();
    m.pa_old = s->pa.get(); m.pb_old = s->pb.get(); m.st_old = s->st_o.get(); m.flag_old = s->flag.get();
    m.rank_e = rank_e.get(); m.rank_l = rank_l.get(); m.pa_new = npa.get(); m.pb_new = npb.get(); m.st_new = nst.get(); m.flag_new = nflag.get();
    m.count = nx.count.get();
    hipLaunchKernelGGL(merge_count_kernel, dim3(blocks_of(nx.P)), dim3(TB), 0, 0, m);
    LPCHK(hipGetLastError());
    std::vector<int> count((size_t)nx.P);
    std::vector<long long> offset((size_t)nx.P);
    LPCHK(fetch(count.data(), nx.count.get(), (size_t)nx.P));
    long long total = 0;
    if (!sweep_scan(count.data(), nx.P, offset.data(), &total) || total != T) { g_err = "the merged pair list does not add up"; return GCSADMM_ERR_HIP; }
    LPCHK(hipMemcpy(nx.offset.get(), offset.data(), sizeof(long long) * offset.size(), hipMemcpyHostToDevice));
    if ((rc = alloc_buffers(&nx, BUF_PAIRS, (size_t)T)) != GCSADMM_OK) return rc;
    m.offset = nx.offset.get(); m.pa = nx.pa.get(); m.pb = nx.pb.get(); m.st = nx.st_o.get(); m.flag = nx.flag.get();
    if (m.T_old > 0) hipLaunchKernelGGL(merge_move_old_kernel, dim3(blocks_of((long)m.T_old)), dim3(TB), 0, 0, m);
    if (Tn > 0) hipLaunchKernelGGL(merge_move_new_kernel, dim3(blocks_of((long)Tn)), dim3(TB), 0, 0, m);
    LPCHK(hipGetLastError());
    LPCHK(hipStreamSynchronize(nullptr));

    commit_regions(s, nx, h_ptr);
    commit_pairs(s, nx, T);
    if (num_new_pairs) *num_new_pairs = Tn;
    if (num_overlapping) *num_overlapping = (int64_t)decided[0];
    if (num_undecided) *num_undecided = (int64_t)decided[1];
    return GCSADMM_OK;
}

int gcsadmm_scene_read_regions(gcsadmm_scene s, double *centers, double *radii, int *center_status, double *lo, double *hi, int *box_status)
{
    USE_SCENE(s);
    if ((centers || radii || center_status) && !s->have_centers) { g_err = "no resident centres: call gcsadmm_scene_centers first"; return GCSADMM_ERR_BAD_ARG; }
    if ((lo || hi) && !s->have_boxes) { g_err = "no resident boxes: call gcsadmm_scene_bounds or gcsadmm_scene_set_boxes first"; return GCSADMM_ERR_BAD_ARG; }
    if (int rc = read_centers(s, centers, radii, center_status)) return rc;
    return read_boxes(s, lo, hi, box_status);
}

int gcsadmm_scene_add_regions(gcsadmm_scene s, int num_new, const int *poly_ptr, const double *poly_A, const double *poly_b,
                              double pad, double tol, double *centers, double *radii, int *center_status,
                              int64_t *num_new_pairs, int64_t *num_overlapping, int64_t *num_undecided)
{
    try {
        return add_regions(s, num_new, poly_ptr, poly_A, poly_b, pad, tol, centers, radii, center_status, num_new_pairs, num_overlapping, num_undecided);
    } catch (const std::bad_alloc &) {      // the host arrays of the checks, the sort and the scans
        g_err = "out of host memory"; return GCSADMM_ERR_NO_MEMORY;
    }
}

static int remove_regions(gcsadmm_scene s, int R, const int *regions, int64_t *num_pairs_left)
{
    USE_SCENE(s);
    if (R < 0 || (R > 0 && !regions)) { g_err = "negative number of regions or null index array"; return GCSADMM_ERR_BAD_ARG; }
    const int n = s->n, P = s->P;
    const size_t un = (size_t)n, uP = (size_t)P;
    std::vector<int> newidx(uP);
    int Q = 0;
    if (!remove_renumber(P, R, regions, newidx.data(), &Q)) { g_err = "region index out of range or given twice"; return GCSADMM_ERR_BAD_ARG; }
    if (num_pairs_left) *num_pairs_left = s->have_pairs ? s->T : 0;
    if (R == 0) return GCSADMM_OK;
    const size_t uQ = (size_t)Q;
    gcsadmm_scene_s nx;
    nx.n = n; nx.P = Q; nx.device = s->device;
    std::vector<int> h_ptr(1, 0);
    for (int p = 0; p < P; ++p) {
        if (newidx[p] < 0) continue;
        const int m = s->h_ptr[(size_t)p + 1] - s->h_ptr[p];
        nx.maxm = std::max(nx.maxm, m);
        h_ptr.push_back(h_ptr.back() + m);
    }
    const size_t rows = (size_t)h_ptr.back();

    // the polytopes and the per-region results: row p to row newidx[p]
    DevBuf<int> d_newidx;
    LPCHK(put(d_newidx, newidx.data(), uP));
    LPCHK(put(nx.ptr, h_ptr.data(), h_ptr.size()));
    LPCHK(nx.A.alloc(rows * un)); LPCHK(nx.b.alloc(rows)); LPCHK(nx.nrm.alloc(rows));
    nx.S = Polys{n, Q, nx.ptr.get(), nx.A.get(), nx.b.get(), nx.nrm.get()};
    int rc = alloc_buffers(&nx, BUF_CEN | BUF_CENTRE_LP | BUF_BOXES | BUF_RESIDENT);
    if (rc != GCSADMM_OK) return rc;
    const dim3 grid(blocks_of(P)), block(TB);
    hipLaunchKernelGGL(compact_polys_kernel, grid, block, 0, 0, s->ptr.get(), nx.ptr.get(), d_newidx.get(), n, P, s->A.get(), s->b.get(), s->nrm.get(),
                       nx.A.get(), nx.b.get(), nx.nrm.get());
    auto compact = [&](auto &src, auto &dst, int width) {
        using V = std::remove_pointer_t<decltype(src.get())>;
        hipLaunchKernelGGL(compact_rows_kernel<V>, grid, block, 0, 0, (const V *)src.get(), dst.get(), (const int *)d_newidx.get(), width, P);
    };
    compact(s->w, nx.w, n + 1); compact(s->cen, nx.cen, n); compact(s->rad, nx.rad, 1); compact(s->st_c, nx.st_c, 1);
    compact(s->lo, nx.lo, n); compact(s->hi, nx.hi, n); compact(s->st_b, nx.st_b, 2 * n);
    LPCHK(hipGetLastError());

    // the pair list: the segments of the old sweep order, without the removed boxes and their pairs
    long long T = 0;
    DevBuf<int> d_kept;
    DevBuf<long long> d_dst;
    if (s->have_pairs) {
        LPCHK(d_kept.alloc(uP));
        EditRemove e{};
        e.P = P; e.newidx = d_newidx.get(); e.order = s->order.get(); e.count_old = s->count.get(); e.offset_old = s->offset.get();
        e.pa_old = s->pa.get(); e.pb_old = s->pb.get(); e.st_old = s->st_o.get(); e.flag_old = s->flag.get(); e.kept = d_kept.get();
        hipLaunchKernelGGL(remove_segment_kernel<false>, grid, block, 0, 0, e);
        LPCHK(hipGetLastError());
        std::vector<int> kept(uP), order(uP), new_order, new_count;
        std::vector<long long> dst(uP, 0), new_offset;
        LPCHK(fetch(kept.data(), d_kept.get(), uP)); LPCHK(fetch(order.data(), s->order.get(), uP));
        for (int i = 0; i < P; ++i) {
            dst[i] = T;
            if (newidx[order[i]] < 0) continue;
            new_order.push_back(newidx[order[i]]); new_count.push_back(kept[i]); new_offset.push_back(T);
            T += kept[i];
        }
        if (Q > 0) {
            LPCHK(hipMemcpy(nx.order.get(), new_order.data(), sizeof(int) * uQ, hipMemcpyHostToDevice));
            LPCHK(hipMemcpy(nx.count.get(), new_count.data(), sizeof(int) * uQ, hipMemcpyHostToDevice));
            LPCHK(hipMemcpy(nx.offset.get(), new_offset.data(), sizeof(long long) * uQ, hipMemcpyHostToDevice));
        }
        LPCHK(put(d_dst, dst.data(), uP));
        if ((rc = alloc_buffers(&nx, BUF_PAIRS, (size_t)T)) != GCSADMM_OK) return rc;
        e.dst = d_dst.get(); e.pa = nx.pa.get(); e.pb = nx.pb.get(); e.st = nx.st_o.get(); e.flag = nx.flag.get();
        hipLaunchKernelGGL(remove_segment_kernel<true>, grid, block, 0, 0, e);
        if (Q > 0)
            hipLaunchKernelGGL(sweep_gather_kernel, dim3(blocks_of(Q)), block, 0, 0, nx.lo.get(), nx.hi.get(), nx.order.get(), n, Q, nx.slo.get(), nx.shi.get());
        LPCHK(hipGetLastError());
    }
    LPCHK(hipStreamSynchronize(nullptr));

    commit_regions(s, nx, h_ptr);
    if (s->have_pairs) commit_pairs(s, nx, T);
    if (num_pairs_left) *num_pairs_left = T;
    return GCSADMM_OK;
}

int gcsadmm_scene_remove_regions(gcsadmm_scene s, int num_removed, const int *regions, int64_t *num_pairs_left)
{
    try {
        return remove_regions(s, num_removed, regions, num_pairs_left);
    } catch (const std::bad_alloc &) {      // the host arrays of the renumbering and the scan
        g_err = "out of host memory"; return GCSADMM_ERR_NO_MEMORY;
    }
}

} // extern "C"

// ---- the region graph of a decided scene, and the query graphs of a batch from it (query_graph_core.h) ----
extern "C" {

static int build_region_graph(gcsadmm_scene s, const unsigned char *overlap, int64_t *num_edges)
{
    USE_SCENE(s);
    if (!s->have_pairs || !s->have_overlaps) { g_err = "the resident pairs are not decided: call gcsadmm_scene_overlaps first"; return GCSADMM_ERR_BAD_ARG; }
    const int P = s->P;
    const long long T = s->T;
    DevBuf<unsigned char> d_flag;
    DevBuf<int> d_count;
    if (overlap) LPCHK(put(d_flag, overlap, (size_t)T));
    LPCHK(d_count.upload(nullptr, (size_t)P));
    RegionBuild g{};
    g.P = P; g.T = T; g.pa = s->pa.get(); g.pb = s->pb.get(); g.flag = overlap ? d_flag.get() : s->flag.get(); g.count = d_count.get();
    if (T > 0) hipLaunchKernelGGL(region_count_kernel, dim3(blocks_of((long)T)), dim3(TB), 0, 0, g);
    LPCHK(hipGetLastError());
    std::vector<int> count((size_t)P);
    std::vector<long long> row_ptr((size_t)P + 1);
    LPCHK(fetch(count.data(), d_count.get(), (size_t)P));
    if (!region_scan(count.data(), P, row_ptr.data())) {      // before the graph is allocated
        g_err = "too many region edges: a query graph's incidences would not fit 32-bit indices"; return GCSADMM_ERR_UNSUPPORTED;
    }
    const long long E = row_ptr[(size_t)P];
    DevBuf<long long> d_row_ptr;
    DevBuf<int> unsorted, tail, head, rev;
    LPCHK(put(d_row_ptr, row_ptr.data(), row_ptr.size()));
    LPCHK(unsorted.alloc((size_t)E)); LPCHK(tail.alloc((size_t)E)); LPCHK(head.alloc((size_t)E)); LPCHK(rev.alloc((size_t)E));
    LPCHK(hipMemset(d_count.get(), 0, sizeof(int) * std::max<size_t>((size_t)P, 1)));
    g.row_ptr = d_row_ptr.get(); g.unsorted = unsorted.get(); g.tail = tail.get(); g.head = head.get(); g.rev = rev.get();
    if (E > 0) {
        hipLaunchKernelGGL(region_scatter_kernel, dim3(blocks_of((long)T)), dim3(TB), 0, 0, g);
        hipLaunchKernelGGL(region_place_kernel, dim3(blocks_of((long)E)), dim3(TB), 0, 0, g, E);
        hipLaunchKernelGGL(region_reverse_kernel, dim3(blocks_of((long)E)), dim3(TB), 0, 0, g, E);
    }
    LPCHK(hipGetLastError());
    LPCHK(hipStreamSynchronize(nullptr));
    std::swap(s->g_row_ptr, d_row_ptr); std::swap(s->g_tail, tail); std::swap(s->g_head, head); std::swap(s->g_rev, rev);
    s->g_edges = E;
    s->have_graph = true;
    if (num_edges) *num_edges = E;
    return GCSADMM_OK;
}

int gcsadmm_scene_build_region_graph(gcsadmm_scene s, const unsigned char *overlap, int64_t *num_edges)
{
    try {
        return build_region_graph(s, overlap, num_edges);
    } catch (const std::bad_alloc &) {      // the host arrays of the scan
        g_err = "out of host memory"; return GCSADMM_ERR_NO_MEMORY;
    }
}

int gcsadmm_scene_read_region_graph(gcsadmm_scene s, int64_t *row_ptr, int *edge_tail, int *edge_head, int *reverse)
{
    USE_SCENE(s);
    if (!s->have_graph) { g_err = "no resident region graph: call gcsadmm_scene_build_region_graph first"; return GCSADMM_ERR_BAD_ARG; }
    static_assert(sizeof(int64_t) == sizeof(long long), "row_ptr is kept as long long");
    LPCHK(download((long long *)row_ptr, s->g_row_ptr));
    LPCHK(download(edge_tail, s->g_tail)); LPCHK(download(edge_head, s->g_head)); LPCHK(download(reverse, s->g_rev));
    return GCSADMM_OK;
}

static int query_graphs(gcsadmm_scene s, int B, const int64_t *term_ptr, const int *term_region, const unsigned char *st_adjacent, int chunk_queries,
                        const int64_t *edge_off, int *edge_tail, int *edge_head, int *inc_ptr, int *inc_edge, int *inc_out, int *edge_inc_tail,
                        int *edge_inc_head)
{
    USE_SCENE(s);
    static_assert(QUERY_BAD_ARG == GCSADMM_ERR_BAD_ARG && QUERY_UNSUPPORTED == GCSADMM_ERR_UNSUPPORTED && QUERY_OK == GCSADMM_OK, "query_check returns the ABI's codes");
    if (!s->have_graph) {
        g_err = "no resident region graph, or one from before an edit: call gcsadmm_scene_build_region_graph first"; return GCSADMM_ERR_BAD_ARG;
    }
    const int P = s->P;
    const QueryBatch host{B, (const long long *)term_ptr, term_region, st_adjacent, (const long long *)edge_off};
    long long max_items = 0;
    if (const int rc = query_check(P, s->g_edges, host, chunk_queries, g_err, &max_items)) return rc;
    if (B == 0) return GCSADMM_OK;
    if (!edge_tail || !edge_head || !inc_ptr || !inc_edge || !inc_out || !edge_inc_tail || !edge_inc_head) { g_err = "null output array"; return GCSADMM_ERR_BAD_ARG; }
    const size_t points = 2 * (size_t)B, hits = (size_t)host.term_ptr[points], V1 = (size_t)P + 3;
    LPCHK(reserve(s->qg_term_ptr, points + 1)); LPCHK(reserve(s->qg_term_region, hits)); LPCHK(reserve(s->qg_st, (size_t)B)); LPCHK(reserve(s->qg_edge_off, (size_t)B + 1));
    LPCHK(hipMemcpy(s->qg_term_ptr.get(), host.term_ptr, sizeof(long long) * (points + 1), hipMemcpyHostToDevice));
    if (hits > 0) LPCHK(hipMemcpy(s->qg_term_region.get(), term_region, sizeof(int) * hits, hipMemcpyHostToDevice));
    LPCHK(hipMemcpy(s->qg_st.get(), st_adjacent, (size_t)B, hipMemcpyHostToDevice));
    LPCHK(hipMemcpy(s->qg_edge_off.get(), host.edge_off, sizeof(long long) * ((size_t)B + 1), hipMemcpyHostToDevice));
    QueryGraphArgs a{};
    a.g = RegionGraph{P, s->g_edges, s->g_row_ptr.get(), s->g_tail.get(), s->g_head.get(), s->g_rev.get()};
    a.q = QueryBatch{B, s->qg_term_ptr.get(), s->qg_term_region.get(), s->qg_st.get(), s->qg_edge_off.get()};
    a.items = max_items;
    const int chunk = query_chunk(P, s->g_edges, chunk_queries);
    for (int first = 0; first < B; first += chunk) {
        const int count = std::min(chunk, B - first);
        const size_t at = (size_t)host.edge_off[first], E = (size_t)(host.edge_off[first + count] - host.edge_off[first]);
        LPCHK(reserve(s->qg_edge_tail, E)); LPCHK(reserve(s->qg_edge_head, E)); LPCHK(reserve(s->qg_inc_ptr, (size_t)count * V1));
        LPCHK(reserve(s->qg_inc_edge, 2 * E)); LPCHK(reserve(s->qg_inc_out, 2 * E)); LPCHK(reserve(s->qg_edge_inc_tail, E)); LPCHK(reserve(s->qg_edge_inc_head, E));
        a.out = QueryArrays{s->qg_edge_tail.get(), s->qg_edge_head.get(), s->qg_inc_ptr.get(), s->qg_inc_edge.get(), s->qg_inc_out.get(),
                            s->qg_edge_inc_tail.get(), s->qg_edge_inc_head.get()};
        a.first = first;
        hipLaunchKernelGGL(query_graph_kernel, dim3((unsigned)((max_items + 255) / 256), (unsigned)count), dim3(256), 0, 0, a);
        LPCHK(hipGetLastError());
        LPCHK(fetch(edge_tail + at, a.out.edge_tail, E)); LPCHK(fetch(edge_head + at, a.out.edge_head, E));
        LPCHK(fetch(inc_ptr + (size_t)first * V1, a.out.inc_ptr, (size_t)count * V1));
        LPCHK(fetch(inc_edge + 2 * at, a.out.inc_edge, 2 * E)); LPCHK(fetch(inc_out + 2 * at, a.out.inc_out, 2 * E));
        LPCHK(fetch(edge_inc_tail + at, a.out.edge_inc_tail, E)); LPCHK(fetch(edge_inc_head + at, a.out.edge_inc_head, E));
    }
    LPCHK(hipStreamSynchronize(nullptr));
    return GCSADMM_OK;
}

int gcsadmm_scene_query_graphs(gcsadmm_scene s, int num_queries, const int64_t *term_ptr, const int *term_region, const unsigned char *st_adjacent,
                               int chunk_queries, const int64_t *edge_off, int *edge_tail, int *edge_head, int *inc_ptr, int *inc_edge, int *inc_out,
                               int *edge_inc_tail, int *edge_inc_head)
{
    try {
        return query_graphs(s, num_queries, term_ptr, term_region, st_adjacent, chunk_queries, edge_off, edge_tail, edge_head, inc_ptr, inc_edge, inc_out,
                            edge_inc_tail, edge_inc_head);
    } catch (const std::bad_alloc &) {      // the text of a refusal
        g_err = "out of host memory"; return GCSADMM_ERR_NO_MEMORY;
    }
}

} // extern "C"
