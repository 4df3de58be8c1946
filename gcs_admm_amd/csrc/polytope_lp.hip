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
// The resident regions also serve the step after the loop (path_restrict_kernel: path_restrict_core.h, on the offsets and sizes
// restrict_plan.h decides), the queries on a decided scene (locate_kernel: point_locate_core.h), its edits (gcsadmm_scene_add_regions,
// gcsadmm_scene_remove_regions: scene_edit_core.h) and the query graphs of a batch (gcsadmm_scene_build_region_graph,
// gcsadmm_scene_query_graphs: query_graph_core.h) and the informed region set of every query (gcsadmm_scene_region_paths,
// gcsadmm_scene_informed_regions: informed_core.h), and the query graphs on those sets alone (gcsadmm_scene_induced_sizes,
// gcsadmm_scene_induced_query_graphs: induced_graph_core.h).
//
// This file is the host side of one translation unit: scene_kernels.h has the __global__ wrappers around the *_core.h headers,
// scene_stage.h which results a scene holds, which of them each call needs and which it ends (the table is there), hip_owners.h
// DevBuf, the owner of every device buffer, and the copies (to_device, to_host, on_device).  Below: the scene's state in groups by
// lifetime, the entry shim, upload and allocation, the launches and the three LP stages, then the entry points.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <memory>
#include <new>
#include <optional>
#include <string>
#include <vector>

#include "gcsadmm.h"
#include "hip_owners.h"
#include "step_args.h"      // dispatch_dim

#include "scene_kernels.h"
#include "scene_stage.h"

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
#define LPRUN(call) do { if (const int rc_ = (call)) return rc_; } while (0)      // a step that reports a status: any but GCSADMM_OK ends the caller with it

using namespace gcsadmm_lp;
using namespace gcsadmm_stage;

// The scene: everything graph construction computes stays in these buffers until it is read, in groups by lifetime.  An edit builds
// a new group of regions and of pairs beside the resident ones and swaps whole groups in, so a member added to a group cannot be
// forgotten there.  Which results are valid is one word of flags beside the groups (scene_stage.h), not in them: a swap keeps it.
struct SceneRegions {                                  // what there is per region; replaced by an edit
    int n = 0, P = 0, maxm = 0;                        // maxm: most rows of one polytope
    DevBuf<int> ptr;                                   // the polytopes: CSR, rows, right-hand sides, norms of the rows
    DevBuf<double> A, b, nrm;
    std::vector<int> h_ptr;                            // the CSR offsets on the host too (a resident scene's: restrict_plan.h reads them)
    DevBuf<double> w, cen, rad;                        // centre LPs: (x, r) records, centres [P][n], radii,
    DevBuf<int> st_c;                                  //   statuses                                             (HAVE_CENTERS)
    DevBuf<double> lo, hi;                             // boxes [P][n]                                           (HAVE_BOXES)
    DevBuf<int> st_b;                                  //   and the statuses of their LPs [P][n][2]
    DevBuf<double> lo0, slo, shi;                      // sweep: first lower bounds, sorted boxes [n][P],
    DevBuf<int> order, count;                          //   sort order, counts,
    DevBuf<long long> offset;                          //   offsets
    DevBuf<unsigned long long> counts;                 // scratch of a narrow phase: the two counts of its decisions
    Polys polys() const { return Polys{n, P, ptr.get(), A.get(), b.get(), nrm.get()}; }
};
struct ScenePairs {                                    // pair list with the narrow phase's statuses and flags; replaced by a sweep or an edit
    DevBuf<int> pa, pb, st_o;                          //                                                        (HAVE_PAIRS; flag, st_o: HAVE_OVERLAPS)
    DevBuf<unsigned char> flag;
    long long T = 0;
};
struct SceneHits {                                     // the hit list of the last locate_points (HAVE_HITS; kept and grown from call to call)
    DevBuf<int> region;
    DevBuf<unsigned char> cls;
    std::vector<int64_t> ptr;                          //   its segments per point (host: the scan runs there)
    bool projected = false;                            //   which kind of call made it: project_points (true) or a locate call
    DevBuf<double> distance, nearest;                  //   project_points: per hit the distance, the nearest point [n],
    DevBuf<int> status, iterations;                    //   the status and the iterations of its solve
    bool clipped = false;                              //   ... or clip_segments (projected and clipped both false: a locate call)
    DevBuf<double> t_in, t_out;                        //   clip_segments: per hit its span; per segment the cover status, the reach
    DevBuf<int> cover, chain_len, chain;               //   and the length of its chain, written at the segment's offset in `chain`
    DevBuf<double> reach;
    std::vector<int> h_chain_len;                      //   (host: read with the counts, the chain offsets of read_cover come from it)
};
struct SceneGraph {                                    // region graph of the decided pairs (HAVE_GRAPH; query_graph_core.h): rows [P + 1],
    DevBuf<long long> row_ptr;
    DevBuf<int> tail, head, rev;                       //   edges by (tail, head) and the id of each one's opposite edge
    DevBuf<double> w;                                  //   distance between the centres of every edge (region_paths: made on first use)
    long long edges = 0;
};
struct LocateScratch {                                 // locate_points / locate_boxes, kept and grown from call to call: the points [num_points][n] (boxes: [num_boxes][2 n]),
    DevBuf<double> points;
    DevBuf<int> count;                                 //   counts and
    DevBuf<long long> offset;                          //   offsets per (point, chunk)
    DevBuf<double> radius;                             //   project_points: the radii [num_points] and the segments of the list
    DevBuf<long long> hit_ptr;                         //   [num_points + 1]
    DevBuf<double> ends;                               //   clip_segments: the far ends of the segments [num_segments][n]
};
struct QueryScratch {                                  // query_graphs, kept and grown from call to call: the caller's arrays,
    DevBuf<long long> term_ptr, edge_off;
    DevBuf<int> term_region;
    DevBuf<unsigned char> st;
    DevBuf<int> edge_tail, edge_head, inc_ptr, inc_edge, inc_out, edge_inc_tail, edge_inc_head;      //   one chunk of results
};
struct InformedScratch {                               // region_paths and informed_regions, kept and grown from call to call:
    DevBuf<double> points, bound;                      //   the caller's arrays,
    DevBuf<long long> term_ptr;
    DevBuf<int> term_region;
    DevBuf<double> d;                                  //   distances of one chunk of queries [chunk][P],
    DevBuf<int> path_region, path_len, status;         //   the results
    DevBuf<double> cost;
    DevBuf<unsigned char> keep;
};
struct InducedScratch {                                // induced_sizes and induced_query_graphs, kept and grown from call to call:
    DevBuf<long long> term_ptr, vertex_off, edge_off;  //   the caller's arrays (keep: the flags of one chunk) and the renumbered
    DevBuf<int> term_region, term_new;                 //   hit lists,
    DevBuf<unsigned char> st, keep;
    DevBuf<InducedQuery> table;                        //   of one chunk: the table of its slabs,
    DevBuf<int> sizes, newidx, kept, deg;              //   the counts and the arrays of the count kernel [chunk][P],
    DevBuf<long long> row_ptr;                         //   the induced graphs with their ranks, one query behind the other
    DevBuf<int> full_ptr, rank, tail, head, rev;       //   (the seven result arrays are QueryScratch's)
    InducedWorkspace workspace() const
    {
        return InducedWorkspace{keep.get(), newidx.get(), kept.get(), deg.get(), row_ptr.get(), full_ptr.get(), rank.get(), tail.get(), head.get(), rev.get()};
    }
};
// A gcsadmm_scene holds one from create to destroy (read: gcsadmm_scene_read_pairs); a batch call (gcsadmm_polytope_*) holds one on
// its stack, with the buffers of its stage.
struct gcsadmm_scene_s {
    int device = 0;
    unsigned have = 0;                                 // HAVE_*: changed by stage_start / stage_finish alone
    SceneRegions reg;
    ScenePairs pairs;
    SceneHits hits;
    SceneGraph graph;
    LocateScratch lq;                                  // (locate_points)
    QueryScratch qg;                                   // (query_graphs)
    InformedScratch inf;                               // (region_paths, informed_regions)
    InducedScratch ig;                                 // (induced_sizes, induced_query_graphs)
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

// The one shim of the entry points: no exception crosses the C ABI, a failed host allocation is a status.
template <class F> int entry(F &&body)
{
    try {
        return body();
    } catch (const std::bad_alloc &) {      // host arrays of the checks, the sorts and the scans, a plan, the text of a refusal
        g_err = "out of host memory"; return GCSADMM_ERR_NO_MEMORY;
    }
}
// ... of every call on a resident scene: the scene's device for the call, the caller's back on return
template <class F> int scene_entry(gcsadmm_scene s, F &&body)
{
    return entry([&]() -> int {
        if (!s) { g_err = "null scene"; return GCSADMM_ERR_BAD_ARG; }
        DeviceGuard device_guard_(s->device);
        LPRUN(guard_status(device_guard_));
        return body();
    });
}
// the results `call` needs are there, or the call is refused with the first that is not (scene_stage.h)
#define NEED(s, call) if (const char *why_ = need((s)->have, call)) { g_err = why_; return GCSADMM_ERR_BAD_ARG; }

// A CSR slice of `count` polytopes in dimension n: every polytope has a row, the slice fits the room left below 2^31 regions and
// rows, no facet normal is zero.  Raises maxm to the most rows of one of them and takes the norms of the rows.
int check_polytopes(int n, int count, const int *poly_ptr, const double *A, long long room_regions, long long room_rows, int &maxm, std::vector<double> &nrm)
{
    if (poly_ptr[0] != 0) { g_err = "poly_ptr[0] != 0"; return GCSADMM_ERR_BAD_ARG; }
    for (int p = 0; p < count; ++p) {
        const int m = poly_ptr[p + 1] - poly_ptr[p];
        if (m < 1) { g_err = "polytope without rows"; return GCSADMM_ERR_BAD_ARG; }
        maxm = std::max(maxm, m);
    }
    if (count > room_regions || poly_ptr[count] > room_rows) { g_err = "more than 2^31 - 1 regions or rows"; return GCSADMM_ERR_UNSUPPORTED; }
    const size_t rows = (size_t)poly_ptr[count];
    nrm.resize(rows);
    for (size_t r = 0; r < rows; ++r) {
        double sq = 0;
        for (int k = 0; k < n; ++k) sq += A[r * n + k] * A[r * n + k];
        if (!(sq > 0.0)) { g_err = "zero facet normal"; return GCSADMM_ERR_BAD_ARG; }
        nrm[r] = std::sqrt(sq);
    }
    return GCSADMM_OK;
}

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
    SceneRegions &r = s.reg;
    std::vector<double> nrm;
    LPRUN(check_polytopes(n, P, poly_ptr, A, INT32_MAX, INT32_MAX, r.maxm, nrm));
    const size_t rows = nrm.size();
    guard.emplace(device);
    LPRUN(guard_status(*guard));
    LPCHK(r.ptr.put(poly_ptr, (size_t)P + 1));
    if (rows > 0) {      // (a scene without regions has no rows and no buffers for them)
        LPCHK(r.A.put(A, rows * n)); LPCHK(r.b.put(b, rows)); LPCHK(r.nrm.put(nrm.data(), rows));
    }
    r.n = n; r.P = P; s.device = device;
    return GCSADMM_OK;
}

// The buffers of the stages are allocated here and nowhere else: gcsadmm_scene_create takes a resident scene's, and
// gcsadmm_scene_candidate_pairs the pair list's once it knows T; a batch call takes those of its one stage.
enum : unsigned {
    BUF_CEN = 1,            // the centres: written by the centre stage, read by the other two
    BUF_CENTRE_LP = 2, BUF_BOXES = 4, BUF_PAIRS = 8,
    BUF_RESIDENT = 16       // the sweep's arrays and the counts of decisions: what only a resident scene has
};
int alloc_buffers(SceneRegions &r, ScenePairs &pr, unsigned which, size_t T = 0)
{
    const size_t P = (size_t)r.P, n = (size_t)r.n;
    hipError_t e = hipSuccess;
    auto take = [&](unsigned group, auto &buf, size_t count) {
        if (!(which & group) || e != hipSuccess) return;
        buf.reset();      // (before the new one is taken: a pair list is replaced, not held twice)
        e = buf.alloc(count);
    };
    take(BUF_CEN, r.cen, P * n);
    take(BUF_CENTRE_LP, r.w, P * (n + 1)); take(BUF_CENTRE_LP, r.rad, P); take(BUF_CENTRE_LP, r.st_c, P);
    take(BUF_BOXES, r.lo, P * n); take(BUF_BOXES, r.hi, P * n); take(BUF_BOXES, r.st_b, P * 2 * n);
    take(BUF_RESIDENT, r.lo0, P); take(BUF_RESIDENT, r.order, P); take(BUF_RESIDENT, r.slo, P * n); take(BUF_RESIDENT, r.shi, P * n);
    take(BUF_RESIDENT, r.count, P); take(BUF_RESIDENT, r.offset, P); take(BUF_RESIDENT, r.counts, 2);
    take(BUF_PAIRS, pr.pa, T); take(BUF_PAIRS, pr.pb, T); take(BUF_PAIRS, pr.flag, T); take(BUF_PAIRS, pr.st_o, T);
    if (e != hipSuccess) { g_err = std::string("hipMalloc: ") + hipGetErrorString(e); return GCSADMM_ERR_HIP; }
    return GCSADMM_OK;
}

// ---- the launches ----
template <int N> int launch_ball(const SceneRegions &r, long count, const int *d_pa, const int *d_pb, const double *d_x0, int rows_max, double tol, int early,
                double *d_w, unsigned char *d_flag, int *d_status)
{
    const size_t lds = lds_bytes(rows_max);
    if (lds > LDS_MAX_BYTES) { g_err = "too many facet rows per LP for LDS"; return GCSADMM_ERR_UNSUPPORTED; }
    LPCHK(hipFuncSetAttribute((const void *)ball_kernel<N>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    if (count > 0)
        hipLaunchKernelGGL(ball_kernel<N>, dim3((unsigned)((count + WAVE - 1) / WAVE)), dim3(WAVE), lds, 0, r.polys(), (int)count, d_pa, d_pb,
                           d_x0, rows_max, tol, early, d_w, d_flag, d_status);
    LPCHK(hipGetLastError());
    return GCSADMM_OK;
}

template <int N> int launch_bounds(const SceneRegions &r, int first, int polys, const double *d_centers, double *d_lo, double *d_hi, int *d_status)
{
    const int rows_max = bounds_rows(r.maxm, N);
    const size_t lds = lds_bytes(rows_max);
    if (lds > LDS_MAX_BYTES) { g_err = "too many facet rows per LP for LDS"; return GCSADMM_ERR_UNSUPPORTED; }
    LPCHK(hipFuncSetAttribute((const void *)bounds_kernel<N>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    const long count = (long)polys * 2 * N;
    if (count > 0)
        hipLaunchKernelGGL(bounds_kernel<N>, dim3((unsigned)((count + WAVE - 1) / WAVE)), dim3(WAVE), lds, 0, r.polys(), first, polys, d_centers, rows_max, d_lo,
                           d_hi, d_status);
    LPCHK(hipGetLastError());
    return GCSADMM_OK;
}

template <int N> int launch_sweep(const SceneRegions &r, const ScenePairs &pr, bool fill, double pad)
{
    const SortedBoxes B{r.P, r.slo.get(), r.shi.get(), r.order.get()};
    if (r.P > 0) {
        if (fill)
            hipLaunchKernelGGL((sweep_kernel<N, true>), dim3((unsigned)r.P), dim3(SWEEP_WAVE), 0, 0, B, pad, nullptr, r.offset.get(), pr.pa.get(),
                               pr.pb.get());
        else
            hipLaunchKernelGGL((sweep_kernel<N, false>), dim3((unsigned)r.P), dim3(SWEEP_WAVE), 0, 0, B, pad, r.count.get(), nullptr, nullptr, nullptr);
    }
    LPCHK(hipGetLastError());
    return GCSADMM_OK;
}

template <int N> int launch_locate(const LocateArgs &args, long long num_points, bool fill)
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

template <int N> int launch_locate_boxes(const LocateBoxArgs &args, long long num_boxes, bool fill)
{
    constexpr long long SLAB = 65535;      // grid.y
    for (long long q0 = 0; q0 < num_boxes; q0 += SLAB) {
        LocateBoxArgs a = args;
        a.first_box = (int)q0;
        const dim3 grid((unsigned)a.chunks, (unsigned)std::min(SLAB, num_boxes - q0));
        if (fill) hipLaunchKernelGGL((locate_box_kernel<N, true>), grid, dim3(LOCATE_WAVE), 0, 0, a);
        else hipLaunchKernelGGL((locate_box_kernel<N, false>), grid, dim3(LOCATE_WAVE), 0, 0, a);
        LPCHK(hipGetLastError());
    }
    return GCSADMM_OK;
}

template <int N> int launch_project_list(const ProjectArgs &args, long long num_points, bool fill)
{
    constexpr long long SLAB = 65535;      // grid.y
    for (long long q0 = 0; q0 < num_points; q0 += SLAB) {
        ProjectArgs a = args;
        a.first_point = (int)q0;
        const dim3 grid((unsigned)a.chunks, (unsigned)std::min(SLAB, num_points - q0));
        if (fill) hipLaunchKernelGGL((project_list_kernel<N, true>), grid, dim3(LOCATE_WAVE), 0, 0, a);
        else hipLaunchKernelGGL((project_list_kernel<N, false>), grid, dim3(LOCATE_WAVE), 0, 0, a);
        LPCHK(hipGetLastError());
    }
    return GCSADMM_OK;
}

template <int N> int launch_project_solve(const ProjectSolveArgs &args)
{
    constexpr long long SLAB = 1LL << 30;      // workgroups of one launch (grid.x)
    const long long groups = (args.total + PROJECT_LANES - 1) / PROJECT_LANES;
    for (long long g0 = 0; g0 < groups; g0 += SLAB) {
        ProjectSolveArgs a = args;
        a.first = g0 * PROJECT_LANES;
        hipLaunchKernelGGL(project_solve_kernel<N>, dim3((unsigned)std::min(SLAB, groups - g0)), dim3(PROJECT_LANES), 0, 0, a);
        LPCHK(hipGetLastError());
    }
    return GCSADMM_OK;
}

template <int N> int launch_clip(const ClipArgs &args, long long num_segments, bool fill)
{
    constexpr long long SLAB = 65535;      // grid.y
    for (long long q0 = 0; q0 < num_segments; q0 += SLAB) {
        ClipArgs a = args;
        a.first_segment = (int)q0;
        const dim3 grid((unsigned)a.chunks, (unsigned)std::min(SLAB, num_segments - q0));
        if (fill) hipLaunchKernelGGL((segment_clip_kernel<N, true>), grid, dim3(LOCATE_WAVE), 0, 0, a);
        else hipLaunchKernelGGL((segment_clip_kernel<N, false>), grid, dim3(LOCATE_WAVE), 0, 0, a);
        LPCHK(hipGetLastError());
    }
    return GCSADMM_OK;
}

int launch_chain(const ChainArgs &args, long long num_segments)
{
    constexpr long long SLAB = 1LL << 30;      // workgroups of one launch (grid.x)
    for (long long q0 = 0; q0 < num_segments; q0 += SLAB) {
        ChainArgs a = args;
        a.first_segment = q0;
        hipLaunchKernelGGL(segment_chain_kernel, dim3((unsigned)std::min(SLAB, num_segments - q0)), dim3(LOCATE_WAVE), 0, 0, a);
        LPCHK(hipGetLastError());
    }
    return GCSADMM_OK;
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

// ---- the three LP stages, on the scene's buffers: what both families of entry points run ----
// centre LPs of all polytopes into w and st_c, then the centres and radii out of the records
int run_centers(SceneRegions &r)
{
    LPRUN(for_dim(r.n, [&](auto N) {
        return launch_ball<decltype(N)::value>(r, r.P, nullptr, nullptr, nullptr, centre_rows(r.maxm), 0.0, 0, r.w.get(), nullptr, r.st_c.get());
    }));
    if (r.P > 0) hipLaunchKernelGGL(split_centres_kernel, dim3(blocks_of(r.P)), dim3(TB), 0, 0, r.w.get(), r.n, r.P, r.cen.get(), r.rad.get());
    LPCHK(hipGetLastError());
    return GCSADMM_OK;
}

// the 2n bound LPs of every polytope, started at cen, into lo, hi and st_b: what the LPs left (a failed side is not opened here)
int run_bounds(SceneRegions &r)
{
    return for_dim(r.n, [&](auto N) { return launch_bounds<decltype(N)::value>(r, 0, r.P, r.cen.get(), r.lo.get(), r.hi.get(), r.st_b.get()); });
}

// one LP per pair of pa, pb into flag and st_o; x0: the scene's centres (LP t starts at x0[pa[t]]), or nullptr (least-squares points)
int run_overlaps(const SceneRegions &r, ScenePairs &pr, const double *x0, double tol)
{
    return for_dim(r.n, [&](auto N) {
        return launch_ball<decltype(N)::value>(r, (long)pr.T, pr.pa.get(), pr.pb.get(), x0, overlap_rows(r.maxm), tol, 1, nullptr, pr.flag.get(),
                                               pr.st_o.get());
    });
}

// the two counts of a narrow phase's decisions (count_decisions_kernel) through the scene's counts
int count_decisions(const SceneRegions &r, const unsigned char *d_flag, const int *d_status, long T, unsigned long long counts[2])
{
    counts[0] = counts[1] = 0;
    LPCHK(to_device(r.counts.get(), counts, 2));
    if (T > 0) hipLaunchKernelGGL(count_decisions_kernel, dim3(blocks_of(T)), dim3(TB), 0, 0, d_flag, d_status, T, r.counts.get());
    LPCHK(hipGetLastError());
    LPCHK(to_host(counts, r.counts));
    return GCSADMM_OK;
}

// ---- their results to the host (a null pointer: not wanted) ----
int read_centers(const SceneRegions &r, double *centers, double *radii, int *status)
{
    LPCHK(to_host(centers, r.cen)); LPCHK(to_host(radii, r.rad)); LPCHK(to_host(status, r.st_c));
    return GCSADMM_OK;
}
int read_boxes(const SceneRegions &r, double *lo, double *hi, int *status)
{
    LPCHK(to_host(lo, r.lo)); LPCHK(to_host(hi, r.hi)); LPCHK(to_host(status, r.st_b));
    return GCSADMM_OK;
}
int read_decisions(const ScenePairs &pr, unsigned char *overlap, int *status)
{
    LPCHK(to_host(overlap, pr.flag)); LPCHK(to_host(status, pr.st_o));
    return GCSADMM_OK;
}

// ---- the induced query graphs of a batch (induced_graph_core.h): what the two entry points share ----
InducedArgs induced_args(const gcsadmm_scene_s &s, int B, int first)
{
    const SceneGraph &rg = s.graph;
    const InducedScratch &w = s.ig;
    InducedArgs a{};
    a.g = RegionGraph{s.reg.P, rg.edges, rg.row_ptr.get(), rg.tail.get(), rg.head.get(), rg.rev.get()};
    a.table = w.table.get();
    a.q = QueryBatch{B, w.term_ptr.get(), w.term_region.get(), w.st.get(), w.edge_off.get()};
    a.term_new = w.term_new.get(); a.first = first; a.sizes = w.sizes.get();
    return a;
}
// the count kernel on the queries first .. first + count: their flags up, the table of the slabs of fixed size, the counts back
int induced_count(gcsadmm_scene_s &s, const InducedBatch &host, int first, int count, int *sizes)
{
    InducedScratch &w = s.ig;
    const size_t cells = (size_t)count * s.reg.P;
    LPCHK(w.keep.reserve(cells)); LPCHK(w.newidx.reserve(cells)); LPCHK(w.kept.reserve(cells)); LPCHK(w.deg.reserve(cells));
    LPCHK(w.table.reserve((size_t)count)); LPCHK(w.sizes.reserve((size_t)INDUCED_SIZES * count));
    LPCHK(to_device(w.keep.get(), host.keep + (size_t)first * s.reg.P, cells));
    std::vector<InducedQuery> table((size_t)count);
    induced_table(w.workspace(), s.reg.P, count, nullptr, table.data());
    LPCHK(to_device(w.table.get(), table.data(), table.size()));
    hipLaunchKernelGGL(induced_count_kernel, dim3((unsigned)count), dim3(INDUCED_TILE), 0, 0, induced_args(s, host.B, first));
    LPCHK(hipGetLastError());
    LPCHK(to_host(sizes, w.sizes.get(), (size_t)INDUCED_SIZES * count));
    return GCSADMM_OK;
}
// The checks that need no count, the hit lists to the device, then the counts of every query [B][INDUCED_SIZES], chunk by chunk (the
// arrays of the count kernel are those of the last chunk afterwards).
int induced_counts(gcsadmm_scene_s &s, const InducedBatch &host, int chunk_queries, int &chunk, std::vector<int> &sizes)
{
    static_assert(QUERY_BAD_ARG == GCSADMM_ERR_BAD_ARG && QUERY_UNSUPPORTED == GCSADMM_ERR_UNSUPPORTED && QUERY_OK == GCSADMM_OK, "induced_check returns the ABI's codes");
    if (!has(s.have, NEED_FRESH_GRAPH.flags)) { g_err = NEED_FRESH_GRAPH.refusal; return GCSADMM_ERR_BAD_ARG; }
    LPRUN(induced_check(s.reg.P, host, chunk_queries, g_err));
    if (host.B == 0) return GCSADMM_OK;
    InducedScratch &w = s.ig;
    const size_t B = (size_t)host.B, hits = (size_t)host.term_ptr[2 * B];
    LPCHK(w.term_ptr.reserve(2 * B + 1)); LPCHK(w.term_region.reserve(hits)); LPCHK(w.term_new.reserve(hits)); LPCHK(w.st.reserve(B));
    LPCHK(to_device(w.term_ptr.get(), host.term_ptr, 2 * B + 1));
    LPCHK(to_device(w.term_region.get(), host.term_region, hits));
    LPCHK(to_device(w.st.get(), host.st, B));
    sizes.resize(INDUCED_SIZES * B);
    chunk = induced_chunk(s.reg.P, s.graph.edges, chunk_queries);
    for (int first = 0; first < host.B; first += chunk)
        LPRUN(induced_count(s, host, first, std::min(chunk, host.B - first), sizes.data() + (size_t)INDUCED_SIZES * first));
    return GCSADMM_OK;
}
// The build and the query kernel on a counted chunk whose count arrays are resident, and its results to the caller's arrays.
int induced_write(gcsadmm_scene_s &s, const InducedBatch &host, int first, int count, const int *sizes, const long long *vertex_off,
                  const long long *edge_off, const QueryArrays &out)
{
    InducedScratch &w = s.ig;
    QueryScratch &qg = s.qg;
    const InducedTotals n = induced_totals(sizes, count);
    LPCHK(w.row_ptr.reserve(n.kept + (size_t)count)); LPCHK(w.full_ptr.reserve(n.kept)); LPCHK(w.rank.reserve(n.ranks));
    LPCHK(w.tail.reserve(n.edges)); LPCHK(w.head.reserve(n.edges)); LPCHK(w.rev.reserve(n.edges));
    std::vector<InducedQuery> table((size_t)count);
    induced_table(w.workspace(), s.reg.P, count, sizes, table.data());
    LPCHK(to_device(w.table.get(), table.data(), table.size()));
    hipLaunchKernelGGL(induced_build_kernel, dim3((unsigned)count), dim3(INDUCED_TILE), 0, 0, induced_args(s, host.B, first));
    LPCHK(hipGetLastError());
    const size_t at = (size_t)edge_off[first], E = (size_t)(edge_off[first + count] - edge_off[first]);
    const size_t v_at = (size_t)vertex_off[first], V = (size_t)(vertex_off[first + count] - vertex_off[first]);
    LPCHK(qg.edge_tail.reserve(E)); LPCHK(qg.edge_head.reserve(E)); LPCHK(qg.inc_ptr.reserve(V));
    LPCHK(qg.inc_edge.reserve(2 * E)); LPCHK(qg.inc_out.reserve(2 * E)); LPCHK(qg.edge_inc_tail.reserve(E)); LPCHK(qg.edge_inc_head.reserve(E));
    InducedGraphArgs a{};
    a.table = w.table.get();
    a.q = QueryBatch{host.B, w.term_ptr.get(), w.term_new.get(), w.st.get(), w.edge_off.get()};
    a.vertex_off = w.vertex_off.get();
    a.out = QueryArrays{qg.edge_tail.get(), qg.edge_head.get(), qg.inc_ptr.get(), qg.inc_edge.get(), qg.inc_out.get(), qg.edge_inc_tail.get(),
                        qg.edge_inc_head.get()};
    a.first = first;
    long long max_items = 0;
    for (int y = 0; y < count; ++y)
        max_items = std::max(max_items, query_items(induced_region_graph(table[(size_t)y]), induced_hits(QueryBatch{host.B, host.term_ptr}, first + y), 0));
    hipLaunchKernelGGL(induced_graph_kernel, dim3((unsigned)((max_items + 255) / 256), (unsigned)count), dim3(256), 0, 0, a);
    LPCHK(hipGetLastError());
    LPCHK(to_host(out.edge_tail + at, a.out.edge_tail, E)); LPCHK(to_host(out.edge_head + at, a.out.edge_head, E));
    LPCHK(to_host(out.inc_ptr + v_at, a.out.inc_ptr, V));
    LPCHK(to_host(out.inc_edge + 2 * at, a.out.inc_edge, 2 * E)); LPCHK(to_host(out.inc_out + 2 * at, a.out.inc_out, 2 * E));
    LPCHK(to_host(out.edge_inc_tail + at, a.out.edge_inc_tail, E)); LPCHK(to_host(out.edge_inc_head + at, a.out.edge_inc_head, E));
    return GCSADMM_OK;
}

} // namespace

extern "C" {

const char *gcsadmm_polytope_last_error(void) { return g_err.c_str(); }

// ---- batch calls: a scene for the length of the call, with the buffers of one stage; host arrays in, host arrays out ----
int gcsadmm_polytope_centers(int n, int num_polytopes, const int *poly_ptr, const double *poly_A, const double *poly_b,
                             int device, double *centers, double *radii, int *status)
{
    return entry([&]() -> int {
        if (!centers) { g_err = "null output"; return GCSADMM_ERR_BAD_ARG; }
        std::optional<DeviceGuard> guard;
        gcsadmm_scene_s s;
        LPRUN(upload_scene(s, guard, n, num_polytopes, poly_ptr, poly_A, poly_b, device));
        LPRUN(alloc_buffers(s.reg, s.pairs, BUF_CEN | BUF_CENTRE_LP));
        LPRUN(run_centers(s.reg));
        return read_centers(s.reg, centers, radii, status);
    });
}

int gcsadmm_polytope_bounds(int n, int num_polytopes, const int *poly_ptr, const double *poly_A, const double *poly_b,
                            const double *centers, int device, double *lo, double *hi, int *status)
{
    return entry([&]() -> int {
        if (!centers || !lo || !hi) { g_err = "null centres or output"; return GCSADMM_ERR_BAD_ARG; }
        std::optional<DeviceGuard> guard;
        gcsadmm_scene_s s;
        LPRUN(upload_scene(s, guard, n, num_polytopes, poly_ptr, poly_A, poly_b, device));
        LPRUN(alloc_buffers(s.reg, s.pairs, BUF_CEN | BUF_BOXES));
        LPCHK(to_device(s.reg.cen.get(), centers, s.reg.cen.size()));
        LPRUN(run_bounds(s.reg));
        return read_boxes(s.reg, lo, hi, status);      // as the LPs left them: opening a failed side is the caller's
    });
}

int gcsadmm_polytope_overlaps(int n, int num_polytopes, const int *poly_ptr, const double *poly_A, const double *poly_b,
                              const double *centers, long num_pairs, const int *pair_a, const int *pair_b, double tol,
                              int device, unsigned char *overlap, int *status)
{
    return entry([&]() -> int {
        if (num_pairs < 0 || (num_pairs > 0 && (!pair_a || !pair_b || !overlap))) { g_err = "null pair list or output"; return GCSADMM_ERR_BAD_ARG; }
        for (long t = 0; t < num_pairs; ++t)
            if (pair_a[t] < 0 || pair_a[t] >= num_polytopes || pair_b[t] < 0 || pair_b[t] >= num_polytopes) {
                g_err = "pair index out of range"; return GCSADMM_ERR_BAD_ARG;
            }
        std::optional<DeviceGuard> guard;
        gcsadmm_scene_s s;
        LPRUN(upload_scene(s, guard, n, num_polytopes, poly_ptr, poly_A, poly_b, device));
        LPRUN(alloc_buffers(s.reg, s.pairs, (centers ? BUF_CEN : 0u) | BUF_PAIRS, (size_t)num_pairs));
        s.pairs.T = num_pairs;
        LPCHK(to_device(s.pairs.pa.get(), pair_a, s.pairs.pa.size()));
        LPCHK(to_device(s.pairs.pb.get(), pair_b, s.pairs.pb.size()));
        LPCHK(to_device(s.reg.cen.get(), centers, s.reg.cen.size()));
        LPRUN(run_overlaps(s.reg, s.pairs, s.reg.cen.get(), tol));      // (no centres: no buffer, every LP starts from its least-squares point)
        return read_decisions(s.pairs, overlap, status);
    });
}

// ---- the resident scene: precondition, stage, what only it does, results, synchronise, flag ----
int gcsadmm_scene_create(int n, int num_polytopes, const int *poly_ptr, const double *poly_A, const double *poly_b, int device,
                         gcsadmm_scene *out)
{
    if (!out) { g_err = "null output"; return GCSADMM_ERR_BAD_ARG; }
    *out = nullptr;
    return entry([&]() -> int {
        std::optional<DeviceGuard> guard;      // (outlives the scene: a scene that is given up releases its buffers on its device)
        std::unique_ptr<gcsadmm_scene_s> s(new gcsadmm_scene_s);
        int rc = upload_scene(*s, guard, n, num_polytopes, poly_ptr, poly_A, poly_b, device);
        if (rc == GCSADMM_OK) s->reg.h_ptr.assign(poly_ptr, poly_ptr + num_polytopes + 1);
        if (rc == GCSADMM_OK) rc = alloc_buffers(s->reg, s->pairs, BUF_CEN | BUF_CENTRE_LP | BUF_BOXES | BUF_RESIDENT);
        if (rc == GCSADMM_OK) *out = s.release();
        return rc;
    });
}

void gcsadmm_scene_destroy(gcsadmm_scene s)
{
    if (!s) return;
    DeviceGuard device_guard_(s->device);
    delete s;
}

int gcsadmm_scene_centers(gcsadmm_scene s, double *centers, double *radii, int *status)
{
    return scene_entry(s, [&]() -> int {
        stage_start(s->have, CALL_CENTERS);
        LPRUN(run_centers(s->reg));
        LPRUN(read_centers(s->reg, centers, radii, status));
        LPCHK(hipStreamSynchronize(nullptr));
        stage_finish(s->have, CALL_CENTERS);
        return GCSADMM_OK;
    });
}

int gcsadmm_scene_bounds(gcsadmm_scene s, double *lo, double *hi, int *status)
{
    return scene_entry(s, [&]() -> int {
        NEED(s, CALL_BOUNDS);
        stage_start(s->have, CALL_BOUNDS);
        SceneRegions &r = s->reg;
        LPRUN(run_bounds(r));
        const long sides = (long)r.P * r.n * 2;
        if (sides > 0) hipLaunchKernelGGL(open_failed_sides_kernel, dim3(blocks_of(sides)), dim3(TB), 0, 0, r.st_b.get(), r.n, r.P, r.lo.get(), r.hi.get());
        LPCHK(hipGetLastError());
        LPRUN(read_boxes(r, lo, hi, status));
        LPCHK(hipStreamSynchronize(nullptr));
        stage_finish(s->have, CALL_BOUNDS);
        return GCSADMM_OK;
    });
}

int gcsadmm_scene_set_boxes(gcsadmm_scene s, const double *lo, const double *hi)
{
    return scene_entry(s, [&]() -> int {
        const size_t cells = (size_t)s->reg.P * s->reg.n;
        if (cells > 0 && (!lo || !hi)) { g_err = "null boxes"; return GCSADMM_ERR_BAD_ARG; }
        for (size_t i = 0; i < cells; ++i)
            if (!(lo[i] <= hi[i])) { g_err = "box with a NaN or with lo > hi"; return GCSADMM_ERR_BAD_ARG; }
        stage_start(s->have, CALL_SET_BOXES);
        LPCHK(to_device(s->reg.lo.get(), lo, cells));
        LPCHK(to_device(s->reg.hi.get(), hi, cells));
        stage_finish(s->have, CALL_SET_BOXES);
        return GCSADMM_OK;
    });
}

int gcsadmm_scene_candidate_pairs(gcsadmm_scene s, double pad, int64_t *num_pairs)
{
    return scene_entry(s, [&]() -> int {
        NEED(s, CALL_CANDIDATE_PAIRS);
        if (!(pad == pad)) { g_err = "pad is NaN"; return GCSADMM_ERR_BAD_ARG; }
        SceneRegions &r = s->reg;
        const int n = r.n, P = r.P;
        stage_start(s->have, CALL_CANDIDATE_PAIRS);
        s->pairs.T = 0;
        // sort on the host (P log P on P doubles; a device radix sort would order -0.0 before +0.0 and change the order of ties)
        std::vector<double> lo0((size_t)P);
        std::vector<int> order((size_t)P), count((size_t)P);
        std::vector<long long> offset((size_t)P);
        if (P > 0) hipLaunchKernelGGL(first_lower_bounds_kernel, dim3(blocks_of(P)), dim3(TB), 0, 0, r.lo.get(), n, P, r.lo0.get());
        LPCHK(hipGetLastError());
        LPCHK(to_host(lo0.data(), r.lo0));
        for (int p = 0; p < P; ++p)      // a NaN has no place in the order (set_boxes refuses one; a bounds LP reports none with a status >= 0)
            if (!(lo0[p] == lo0[p])) { g_err = "resident box with a NaN lower bound"; return GCSADMM_ERR_BAD_ARG; }
        sweep_order(lo0.data(), P, order.data());
        LPCHK(to_device(r.order.get(), order.data(), (size_t)P));
        if (P > 0)
            hipLaunchKernelGGL(sweep_gather_kernel, dim3(blocks_of(P)), dim3(TB), 0, 0, r.lo.get(), r.hi.get(), r.order.get(), n, P, r.slo.get(), r.shi.get());
        LPCHK(hipGetLastError());
        LPRUN(for_dim(n, [&](auto N) { return launch_sweep<decltype(N)::value>(r, s->pairs, false, pad); }));
        LPCHK(to_host(count.data(), r.count));
        long long total = 0;
        if (!sweep_scan(count.data(), P, offset.data(), &total)) {      // before anything is allocated
            g_err = "more than 2^31 - 1 candidate pairs"; return GCSADMM_ERR_UNSUPPORTED;
        }
        LPRUN(alloc_buffers(r, s->pairs, BUF_PAIRS, (size_t)total));
        LPCHK(to_device(r.offset.get(), offset.data(), (size_t)P));
        if (total > 0) LPRUN(for_dim(n, [&](auto N) { return launch_sweep<decltype(N)::value>(r, s->pairs, true, pad); }));
        LPCHK(hipStreamSynchronize(nullptr));
        s->pairs.T = total;
        stage_finish(s->have, CALL_CANDIDATE_PAIRS);
        if (num_pairs) *num_pairs = total;
        return GCSADMM_OK;
    });
}

int gcsadmm_scene_overlaps(gcsadmm_scene s, double tol, int64_t *num_overlapping, int64_t *num_undecided)
{
    return scene_entry(s, [&]() -> int {
        NEED(s, CALL_OVERLAPS);
        stage_start(s->have, CALL_OVERLAPS);
        LPRUN(run_overlaps(s->reg, s->pairs, s->reg.cen.get(), tol));
        if (num_overlapping || num_undecided) {      // counted where the flags are: two numbers come back, the arrays stay for read_pairs
            unsigned long long counts[2];
            LPRUN(count_decisions(s->reg, s->pairs.flag.get(), s->pairs.st_o.get(), (long)s->pairs.T, counts));
            if (num_overlapping) *num_overlapping = (int64_t)counts[0];
            if (num_undecided) *num_undecided = (int64_t)counts[1];
        }
        LPCHK(hipStreamSynchronize(nullptr));
        stage_finish(s->have, CALL_OVERLAPS);
        return GCSADMM_OK;
    });
}

int gcsadmm_scene_read_pairs(gcsadmm_scene s, int *pair_a, int *pair_b, unsigned char *overlap, int *status)
{
    return scene_entry(s, [&]() -> int {
        NEED(s, (overlap || status) ? CALL_READ_DECISIONS : CALL_READ_PAIRS);
        LPCHK(to_host(pair_a, s->pairs.pa)); LPCHK(to_host(pair_b, s->pairs.pb));
        return read_decisions(s->pairs, overlap, status);
    });
}

int gcsadmm_scene_read_regions(gcsadmm_scene s, double *centers, double *radii, int *center_status, double *lo, double *hi, int *box_status)
{
    return scene_entry(s, [&]() -> int {
        if (centers || radii || center_status) NEED(s, CALL_READ_CENTERS);
        if (lo || hi) NEED(s, CALL_READ_BOXES);
        LPRUN(read_centers(s->reg, centers, radii, center_status));
        return read_boxes(s->reg, lo, hi, box_status);
    });
}

int gcsadmm_scene_restrict_paths(gcsadmm_scene s, int num_paths, const int *path_ptr, const int *path_poly, const double *start, double tol,
                                 int max_iter, double *points, double *cost, int *iterations, int *status)
{
    return scene_entry(s, [&]() -> int {
        const SceneRegions &r = s->reg;
        gcsadmm_k::RestrictPlan rp;
        LPRUN(gcsadmm_k::make_restrict_plan(r.n, r.P, r.h_ptr.data(), num_paths, path_ptr, path_poly, rp, g_err));
        if (!(tol > 0.0) || max_iter < 0) { g_err = "tol must be positive and max_iter non-negative"; return GCSADMM_ERR_BAD_ARG; }
        if (num_paths == 0) return GCSADMM_OK;
        if (!start) { g_err = "null start"; return GCSADMM_ERR_BAD_ARG; }
        const size_t coords = (size_t)rp.total_points * r.n;
        DevBuf<int> d_path_ptr, d_path_poly, d_prefix, d_iterations, d_status;
        DevBuf<long long> d_ws_off;
        DevBuf<double> d_ws, d_start, d_points, d_cost;
        LPCHK(d_path_ptr.put(path_ptr, (size_t)num_paths + 1));
        LPCHK(d_path_poly.put(path_poly, (size_t)rp.total_regions));
        LPCHK(d_prefix.put(rp.row_prefix.data(), rp.row_prefix.size()));
        LPCHK(d_ws_off.put(rp.ws_off.data(), rp.ws_off.size()));
        LPCHK(d_start.put(start, coords));
        LPCHK(d_ws.alloc((size_t)rp.ws_doubles));
        LPCHK(d_points.alloc(coords)); LPCHK(d_cost.alloc((size_t)num_paths));
        LPCHK(d_iterations.alloc((size_t)num_paths)); LPCHK(d_status.alloc((size_t)num_paths));
        const RestrictArgs a{r.ptr.get(), r.A.get(), r.b.get(), d_path_ptr.get(), d_path_poly.get(), d_prefix.get(), d_ws_off.get(), d_ws.get(),
                             d_start.get(), d_points.get(), d_cost.get(), d_iterations.get(), d_status.get(), tol, max_iter, num_paths};
        LPRUN(for_dim(r.n, [&](auto N) -> int {
            hipLaunchKernelGGL(path_restrict_kernel<decltype(N)::value>, dim3((unsigned)rp.grid), dim3((unsigned)rp.threads), 0, 0, a);
            LPCHK(hipGetLastError());
            return GCSADMM_OK;
        }));
        LPCHK(to_host(points, d_points)); LPCHK(to_host(cost, d_cost)); LPCHK(to_host(iterations, d_iterations)); LPCHK(to_host(status, d_status));
        LPCHK(hipStreamSynchronize(nullptr));
        return GCSADMM_OK;
    });
}

int gcsadmm_scene_locate_points(gcsadmm_scene s, int num_points, const double *points, double eps, double tol, int64_t *num_hits)
{
    return scene_entry(s, [&]() -> int {
        const SceneRegions &r = s->reg;
        LocateScratch &lq = s->lq;
        if (num_points < 0 || (num_points > 0 && !points)) { g_err = "negative number of points or null points"; return GCSADMM_ERR_BAD_ARG; }
        if (!(eps >= 0.0) || !(tol >= 0.0) || std::isinf(eps) || std::isinf(tol)) { g_err = "eps and tol must be finite and non-negative"; return GCSADMM_ERR_BAD_ARG; }
        const size_t coords = (size_t)num_points * r.n;
        for (size_t i = 0; i < coords; ++i)
            if (!std::isfinite(points[i])) { g_err = "point with a NaN or an inf coordinate"; return GCSADMM_ERR_BAD_ARG; }
        stage_start(s->have, CALL_LOCATE_POINTS);
        const long long Q = num_points, chunks = locate_chunks(r.P);
        const size_t cells = (size_t)(Q * chunks);
        std::vector<int> count(cells);
        std::vector<long long> offset(cells);
        std::vector<int64_t> hit_ptr((size_t)Q + 1, 0);
        LocateArgs a{};
        a.R = LocateRegions{r.P, r.ptr.get(), r.A.get(), r.b.get()};
        a.margin = eps + 2.0 * tol;
        a.chunks = chunks;
        long long total = 0;
        if (cells > 0) {
            LPCHK(lq.points.reserve(coords)); LPCHK(lq.count.reserve(cells));
            LPCHK(to_device(lq.points.get(), points, coords));
            a.points = lq.points.get(); a.count = lq.count.get();
            LPRUN(for_dim(r.n, [&](auto N) { return launch_locate<decltype(N)::value>(a, Q, false); }));
            LPCHK(to_host(count.data(), lq.count.get(), cells));
            if (!locate_scan(count.data(), Q, chunks, offset.data(), hit_ptr.data())) {      // before the list is allocated
                g_err = "more than 2^31 - 1 hits"; return GCSADMM_ERR_UNSUPPORTED;
            }
            total = hit_ptr[(size_t)Q];
        }
        if (total > 0) {
            LPCHK(s->hits.region.reserve((size_t)total)); LPCHK(s->hits.cls.reserve((size_t)total)); LPCHK(lq.offset.reserve(cells));
            LPCHK(to_device(lq.offset.get(), offset.data(), cells));
            a.offset = lq.offset.get(); a.limit = total;
            a.hit_region = s->hits.region.get(); a.hit_class = s->hits.cls.get();
            LPRUN(for_dim(r.n, [&](auto N) { return launch_locate<decltype(N)::value>(a, Q, true); }));
        }
        LPCHK(hipStreamSynchronize(nullptr));
        s->hits.ptr.swap(hit_ptr);
        s->hits.projected = false;
        s->hits.clipped = false;
        stage_finish(s->have, CALL_LOCATE_POINTS);
        if (num_hits) *num_hits = total;
        return GCSADMM_OK;
    });
}

// locate_points for boxes: the same resident hit list (the stage rule of locate_points), from locate_box_kernel
int gcsadmm_scene_locate_boxes(gcsadmm_scene s, int num_boxes, const double *lo, const double *hi, double tol, int64_t *num_hits)
{
    return scene_entry(s, [&]() -> int {
        const SceneRegions &r = s->reg;
        LocateScratch &lq = s->lq;
        if (num_boxes < 0 || (num_boxes > 0 && (!lo || !hi))) { g_err = "negative number of boxes or null bounds"; return GCSADMM_ERR_BAD_ARG; }
        if (!(tol >= 0.0) || std::isinf(tol)) { g_err = "tol must be finite and non-negative"; return GCSADMM_ERR_BAD_ARG; }
        const size_t n = (size_t)r.n, coords = (size_t)num_boxes * n;
        for (size_t i = 0; i < coords; ++i) {
            if (!std::isfinite(lo[i]) || !std::isfinite(hi[i])) { g_err = "box with a NaN or an inf bound"; return GCSADMM_ERR_BAD_ARG; }
            if (lo[i] > hi[i]) { g_err = "box with lo > hi"; return GCSADMM_ERR_BAD_ARG; }
        }
        stage_start(s->have, CALL_LOCATE_POINTS);
        const long long Q = num_boxes, chunks = locate_chunks(r.P);
        const size_t cells = (size_t)(Q * chunks);
        std::vector<int> count(cells);
        std::vector<long long> offset(cells);
        std::vector<int64_t> hit_ptr((size_t)Q + 1, 0);
        std::vector<double> boxes(2 * coords);
        for (size_t q = 0; q < (size_t)Q; ++q) locate_box_prepare(r.n, lo + q * n, hi + q * n, tol, boxes.data() + q * 2 * n);
        LocateBoxArgs a{};
        a.R = LocateRegions{r.P, r.ptr.get(), r.A.get(), r.b.get()};
        a.chunks = chunks;
        long long total = 0;
        if (cells > 0) {
            LPCHK(lq.points.reserve(2 * coords)); LPCHK(lq.count.reserve(cells));
            LPCHK(to_device(lq.points.get(), boxes.data(), 2 * coords));
            a.boxes = lq.points.get(); a.count = lq.count.get();
            LPRUN(for_dim(r.n, [&](auto N) { return launch_locate_boxes<decltype(N)::value>(a, Q, false); }));
            LPCHK(to_host(count.data(), lq.count.get(), cells));
            if (!locate_scan(count.data(), Q, chunks, offset.data(), hit_ptr.data())) {      // before the list is allocated
                g_err = "more than 2^31 - 1 hits"; return GCSADMM_ERR_UNSUPPORTED;
            }
            total = hit_ptr[(size_t)Q];
        }
        if (total > 0) {
            LPCHK(s->hits.region.reserve((size_t)total)); LPCHK(s->hits.cls.reserve((size_t)total)); LPCHK(lq.offset.reserve(cells));
            LPCHK(to_device(lq.offset.get(), offset.data(), cells));
            a.offset = lq.offset.get(); a.limit = total;
            a.hit_region = s->hits.region.get(); a.hit_class = s->hits.cls.get();
            LPRUN(for_dim(r.n, [&](auto N) { return launch_locate_boxes<decltype(N)::value>(a, Q, true); }));
        }
        LPCHK(hipStreamSynchronize(nullptr));
        s->hits.ptr.swap(hit_ptr);
        s->hits.projected = false;
        s->hits.clipped = false;
        stage_finish(s->have, CALL_LOCATE_POINTS);
        if (num_hits) *num_hits = total;
        return GCSADMM_OK;
    });
}

int gcsadmm_scene_read_hits(gcsadmm_scene s, int64_t *hit_ptr, int *hit_region, unsigned char *hit_class)
{
    return scene_entry(s, [&]() -> int {
        NEED(s, CALL_READ_HITS);
        const SceneHits &h = s->hits;
        if (hit_ptr) std::copy(h.ptr.begin(), h.ptr.end(), hit_ptr);
        const size_t total = (size_t)h.ptr.back();      // (the buffers may be longer: they are kept from call to call)
        LPCHK(to_host(hit_region, h.region.get(), total));
        LPCHK(to_host(hit_class, h.cls.get(), total));
        return GCSADMM_OK;
    });
}

// The nearest regions of points that may lie in none (point_project_core.h): the candidates of every point as the resident hit list
// (the stage rule of locate_points: it replaces the list of a locate call and is replaced by one), then one solve per entry
int gcsadmm_scene_project_points(gcsadmm_scene s, int num_points, const double *points, const double *radius, int max_iter, int64_t *num_hits)
{
    return scene_entry(s, [&]() -> int {
        const SceneRegions &r = s->reg;
        LocateScratch &lq = s->lq;
        SceneHits &h = s->hits;
        if (num_points < 0 || (num_points > 0 && !points)) { g_err = "negative number of points or null points"; return GCSADMM_ERR_BAD_ARG; }
        if (max_iter < 0) { g_err = "max_iter must not be negative"; return GCSADMM_ERR_BAD_ARG; }
        const size_t coords = (size_t)num_points * r.n;
        for (size_t i = 0; i < coords; ++i)
            if (!std::isfinite(points[i])) { g_err = "point with a NaN or an inf coordinate"; return GCSADMM_ERR_BAD_ARG; }
        for (int q = 0; radius && q < num_points; ++q)
            if (!(radius[q] >= 0.0)) { g_err = "radius of point " + std::to_string(q) + " is NaN or negative"; return GCSADMM_ERR_BAD_ARG; }
        stage_start(s->have, CALL_LOCATE_POINTS);
        const long long Q = num_points, chunks = locate_chunks(r.P);
        const size_t cells = (size_t)(Q * chunks);
        std::vector<int> count(cells);
        std::vector<long long> offset(cells);
        std::vector<int64_t> hit_ptr((size_t)Q + 1, 0);
        std::vector<double> rad((size_t)Q, INFINITY);      // (a null radius: +inf for every point)
        if (radius) rad.assign(radius, radius + Q);
        ProjectArgs a{};
        a.R = LocateRegions{r.P, r.ptr.get(), r.A.get(), r.b.get()};
        a.chunks = chunks;
        long long total = 0;
        if (cells > 0) {
            LPCHK(lq.points.reserve(coords)); LPCHK(lq.radius.reserve((size_t)Q)); LPCHK(lq.count.reserve(cells));
            LPCHK(to_device(lq.points.get(), points, coords)); LPCHK(to_device(lq.radius.get(), rad.data(), (size_t)Q));
            a.points = lq.points.get(); a.radius = lq.radius.get(); a.count = lq.count.get();
            LPRUN(for_dim(r.n, [&](auto N) { return launch_project_list<decltype(N)::value>(a, Q, false); }));
            LPCHK(to_host(count.data(), lq.count.get(), cells));
            if (!locate_scan(count.data(), Q, chunks, offset.data(), hit_ptr.data())) {      // before the list is allocated
                g_err = "more than 2^31 - 1 candidates"; return GCSADMM_ERR_UNSUPPORTED;
            }
            total = hit_ptr[(size_t)Q];
        }
        if (total > 0) {
            const size_t T = (size_t)total;
            LPCHK(h.region.reserve(T)); LPCHK(h.cls.reserve(T)); LPCHK(lq.offset.reserve(cells)); LPCHK(lq.hit_ptr.reserve((size_t)Q + 1));
            LPCHK(h.distance.reserve(T)); LPCHK(h.nearest.reserve(T * r.n)); LPCHK(h.status.reserve(T)); LPCHK(h.iterations.reserve(T));
            const std::vector<long long> segments(hit_ptr.begin(), hit_ptr.end());
            LPCHK(to_device(lq.offset.get(), offset.data(), cells)); LPCHK(to_device(lq.hit_ptr.get(), segments.data(), (size_t)Q + 1));
            a.offset = lq.offset.get(); a.limit = total;
            a.hit_region = h.region.get(); a.hit_class = h.cls.get();
            LPRUN(for_dim(r.n, [&](auto N) { return launch_project_list<decltype(N)::value>(a, Q, true); }));
            ProjectSolveArgs v{};
            v.R = a.R; v.points = a.points; v.radius = a.radius; v.hit_ptr = lq.hit_ptr.get(); v.num_points = Q; v.total = total;
            v.hit_region = h.region.get(); v.max_iter = max_iter;
            v.out = ProjectOut{h.distance.get(), h.nearest.get(), h.status.get(), h.iterations.get()};
            LPRUN(for_dim(r.n, [&](auto N) { return launch_project_solve<decltype(N)::value>(v); }));
        }
        LPCHK(hipStreamSynchronize(nullptr));
        h.ptr.swap(hit_ptr);
        h.projected = true;
        h.clipped = false;
        stage_finish(s->have, CALL_LOCATE_POINTS);
        if (num_hits) *num_hits = total;
        return GCSADMM_OK;
    });
}

int gcsadmm_scene_read_projections(gcsadmm_scene s, double *distance, double *nearest, int *status, int *iterations)
{
    return scene_entry(s, [&]() -> int {
        NEED(s, CALL_READ_HITS);
        const SceneHits &h = s->hits;
        if (!h.projected) { g_err = "the resident hit list is a locate call's: call gcsadmm_scene_project_points first"; return GCSADMM_ERR_BAD_ARG; }
        const size_t total = (size_t)h.ptr.back();      // (the buffers may be longer: they are kept from call to call)
        LPCHK(to_host(distance, h.distance.get(), total)); LPCHK(to_host(nearest, h.nearest.get(), total * s->reg.n));
        LPCHK(to_host(status, h.status.get(), total)); LPCHK(to_host(iterations, h.iterations.get(), total));
        return GCSADMM_OK;
    });
}

// The regions every segment runs through with their spans, and the cover test (segment_clip_core.h): the hits as the resident hit list
// (the stage rule of locate_points: it replaces the list of a locate or project call and is replaced by one), then one wavefront per
// segment for its chain
int gcsadmm_scene_clip_segments(gcsadmm_scene s, int num_segments, const double *from, const double *to, double tol, int64_t *num_hits,
                                int64_t *num_chain)
{
    return scene_entry(s, [&]() -> int {
        const SceneRegions &r = s->reg;
        LocateScratch &lq = s->lq;
        SceneHits &h = s->hits;
        if (num_segments < 0 || (num_segments > 0 && (!from || !to))) { g_err = "negative number of segments or null end points"; return GCSADMM_ERR_BAD_ARG; }
        if (!(tol >= 0.0) || std::isinf(tol)) { g_err = "tol must be finite and non-negative"; return GCSADMM_ERR_BAD_ARG; }
        const size_t coords = (size_t)num_segments * r.n;
        for (size_t i = 0; i < coords; ++i)
            if (!std::isfinite(from[i]) || !std::isfinite(to[i])) { g_err = "segment with a NaN or an inf coordinate"; return GCSADMM_ERR_BAD_ARG; }
        stage_start(s->have, CALL_LOCATE_POINTS);
        const long long Q = num_segments, chunks = locate_chunks(r.P);
        const size_t cells = (size_t)(Q * chunks);
        std::vector<int> count(cells), chain_len((size_t)Q, 0);
        std::vector<long long> offset(cells);
        std::vector<int64_t> hit_ptr((size_t)Q + 1, 0);
        ClipArgs a{};
        a.R = LocateRegions{r.P, r.ptr.get(), r.A.get(), r.b.get()};
        a.tol = tol;
        a.chunks = chunks;
        long long total = 0, links = 0;
        if (cells > 0) {
            LPCHK(lq.points.reserve(coords)); LPCHK(lq.ends.reserve(coords)); LPCHK(lq.count.reserve(cells));
            LPCHK(to_device(lq.points.get(), from, coords)); LPCHK(to_device(lq.ends.get(), to, coords));
            a.from = lq.points.get(); a.to = lq.ends.get(); a.count = lq.count.get();
            LPRUN(for_dim(r.n, [&](auto N) { return launch_clip<decltype(N)::value>(a, Q, false); }));
            LPCHK(to_host(count.data(), lq.count.get(), cells));
            if (!locate_scan(count.data(), Q, chunks, offset.data(), hit_ptr.data())) {      // before the list is allocated
                g_err = "more than 2^31 - 1 hits"; return GCSADMM_ERR_UNSUPPORTED;
            }
            total = hit_ptr[(size_t)Q];
        }
        if (Q > 0) {
            const size_t T = (size_t)total;
            LPCHK(h.region.reserve(T)); LPCHK(h.cls.reserve(T)); LPCHK(h.t_in.reserve(T)); LPCHK(h.t_out.reserve(T)); LPCHK(h.chain.reserve(T));
            LPCHK(h.cover.reserve((size_t)Q)); LPCHK(h.reach.reserve((size_t)Q)); LPCHK(h.chain_len.reserve((size_t)Q));
            LPCHK(lq.hit_ptr.reserve((size_t)Q + 1));
            const std::vector<long long> segments(hit_ptr.begin(), hit_ptr.end());
            LPCHK(to_device(lq.hit_ptr.get(), segments.data(), (size_t)Q + 1));
            if (total > 0) {
                LPCHK(lq.offset.reserve(cells));
                LPCHK(to_device(lq.offset.get(), offset.data(), cells));
                a.offset = lq.offset.get(); a.limit = total;
                a.hit_region = h.region.get(); a.hit_class = h.cls.get(); a.hit_in = h.t_in.get(); a.hit_out = h.t_out.get();
                LPRUN(for_dim(r.n, [&](auto N) { return launch_clip<decltype(N)::value>(a, Q, true); }));
            }
            ChainArgs c{};      // (a segment without hits: a gap at 0, written by its wavefront)
            c.hit_ptr = lq.hit_ptr.get(); c.hit_in = h.t_in.get(); c.hit_out = h.t_out.get();
            c.status = h.cover.get(); c.reach = h.reach.get(); c.chain_len = h.chain_len.get(); c.chain_hit = h.chain.get();
            LPRUN(launch_chain(c, Q));
            LPCHK(to_host(chain_len.data(), h.chain_len.get(), (size_t)Q));
            for (int len : chain_len) links += len;
        }
        LPCHK(hipStreamSynchronize(nullptr));
        h.ptr.swap(hit_ptr);
        h.h_chain_len.swap(chain_len);
        h.projected = false;
        h.clipped = true;
        stage_finish(s->have, CALL_LOCATE_POINTS);
        if (num_hits) *num_hits = total;
        if (num_chain) *num_chain = links;
        return GCSADMM_OK;
    });
}

int gcsadmm_scene_read_spans(gcsadmm_scene s, double *t_in, double *t_out)
{
    return scene_entry(s, [&]() -> int {
        NEED(s, CALL_READ_HITS);
        const SceneHits &h = s->hits;
        if (!h.clipped) { g_err = "the resident hit list is not a clip call's: call gcsadmm_scene_clip_segments first"; return GCSADMM_ERR_BAD_ARG; }
        const size_t total = (size_t)h.ptr.back();      // (the buffers may be longer: they are kept from call to call)
        LPCHK(to_host(t_in, h.t_in.get(), total)); LPCHK(to_host(t_out, h.t_out.get(), total));
        return GCSADMM_OK;
    });
}

int gcsadmm_scene_read_cover(gcsadmm_scene s, int *status, double *reach, int64_t *chain_ptr, int *chain_hit)
{
    return scene_entry(s, [&]() -> int {
        NEED(s, CALL_READ_HITS);
        const SceneHits &h = s->hits;
        if (!h.clipped) { g_err = "the resident hit list is not a clip call's: call gcsadmm_scene_clip_segments first"; return GCSADMM_ERR_BAD_ARG; }
        const size_t Q = h.ptr.size() - 1, total = (size_t)h.ptr.back();
        LPCHK(to_host(status, h.cover.get(), Q)); LPCHK(to_host(reach, h.reach.get(), Q));
        std::vector<int> chain(total);      // every chain at its segment's offset in the list: packed here, segment by segment
        LPCHK(to_host(chain.data(), h.chain.get(), total));
        int64_t at = 0;
        for (size_t q = 0; q < Q; ++q) {
            if (chain_ptr) chain_ptr[q] = at;
            if (chain_hit) std::copy_n(chain.begin() + h.ptr[q], h.h_chain_len[q], chain_hit + at);
            at += h.h_chain_len[q];
        }
        if (chain_ptr) chain_ptr[Q] = at;
        return GCSADMM_OK;
    });
}

// ---- edits of a decided scene: the regions and the pairs are built in groups of their own beside the resident ones, and take their
// place at the end, after the last step that can fail ----
int gcsadmm_scene_add_regions(gcsadmm_scene s, int K, const int *poly_ptr, const double *A, const double *b, double pad, double tol,
                              double *centers, double *radii, int *center_status, int64_t *num_new_pairs, int64_t *num_overlapping,
                              int64_t *num_undecided)
{
    return scene_entry(s, [&]() -> int {
        NEED(s, CALL_ADD_REGIONS);
        if (K < 0 || !poly_ptr || (K > 0 && (!A || !b))) { g_err = "negative number of regions or null polytope array"; return GCSADMM_ERR_BAD_ARG; }
        if (!(pad == pad)) { g_err = "pad is NaN"; return GCSADMM_ERR_BAD_ARG; }
        const SceneRegions &old = s->reg;
        const ScenePairs &oldp = s->pairs;
        const int n = old.n, P = old.P;
        const size_t un = (size_t)n, uP = (size_t)P, uK = (size_t)K;
        const size_t old_rows = (size_t)old.h_ptr[uP];
        SceneRegions nx;
        ScenePairs nxp;
        nx.n = n; nx.maxm = old.maxm;
        std::vector<double> nrm;
        LPRUN(check_polytopes(n, K, poly_ptr, A, (long long)INT32_MAX - P, (long long)INT32_MAX - (long long)old_rows, nx.maxm, nrm));
        const size_t rows = old_rows + nrm.size();
        if (num_new_pairs) *num_new_pairs = 0;
        if (num_overlapping) *num_overlapping = 0;
        if (num_undecided) *num_undecided = 0;
        if (K == 0) return GCSADMM_OK;
        nx.P = P + K;
        nx.h_ptr = old.h_ptr;
        std::vector<int> appended(uK);
        for (int p = 1; p <= K; ++p) nx.h_ptr.push_back((int)old_rows + poly_ptr[p]);
        for (int p = 0; p < K; ++p) appended[p] = P + p;

        // the polytopes and the results of the resident regions
        LPCHK(nx.ptr.put(nx.h_ptr.data(), nx.h_ptr.size()));
        LPCHK(nx.A.alloc(rows * un)); LPCHK(on_device(nx.A.get(), old.A.get(), old_rows * un)); LPCHK(to_device(nx.A.get() + old_rows * un, A, (rows - old_rows) * un));
        LPCHK(nx.b.alloc(rows)); LPCHK(on_device(nx.b.get(), old.b.get(), old_rows)); LPCHK(to_device(nx.b.get() + old_rows, b, rows - old_rows));
        LPCHK(nx.nrm.alloc(rows)); LPCHK(on_device(nx.nrm.get(), old.nrm.get(), old_rows)); LPCHK(to_device(nx.nrm.get() + old_rows, nrm.data(), rows - old_rows));
        LPRUN(alloc_buffers(nx, nxp, BUF_CEN | BUF_CENTRE_LP | BUF_BOXES | BUF_RESIDENT));
        LPCHK(on_device(nx.w.get(), old.w.get(), uP * (un + 1))); LPCHK(on_device(nx.cen.get(), old.cen.get(), uP * un));
        LPCHK(on_device(nx.rad.get(), old.rad.get(), uP)); LPCHK(on_device(nx.st_c.get(), old.st_c.get(), uP));
        LPCHK(on_device(nx.lo.get(), old.lo.get(), uP * un)); LPCHK(on_device(nx.hi.get(), old.hi.get(), uP * un)); LPCHK(on_device(nx.st_b.get(), old.st_b.get(), uP * 2 * un));

        // centre LPs of the new regions; a region without a centre or without interior ends the call, the resident scene untouched
        DevBuf<int> d_appended;
        LPCHK(d_appended.put(appended.data(), uK));
        LPRUN(for_dim(n, [&](auto N) {
            return launch_ball<decltype(N)::value>(nx, K, d_appended.get(), nullptr, nullptr, centre_rows(nx.maxm), 0.0, 0, nx.w.get() + uP * (un + 1), nullptr,
                                                   nx.st_c.get() + uP);
        }));
        hipLaunchKernelGGL(split_centres_kernel, dim3(blocks_of(K)), dim3(TB), 0, 0, nx.w.get() + uP * (un + 1), n, K, nx.cen.get() + uP * un, nx.rad.get() + uP);
        LPCHK(hipGetLastError());
        std::vector<double> rad(uK);
        std::vector<int> st_c(uK);
        LPCHK(to_host(rad.data(), nx.rad.get() + uP, uK)); LPCHK(to_host(st_c.data(), nx.st_c.get() + uP, uK));
        LPCHK(to_host(centers, nx.cen.get() + uP * un, uK * un));
        if (radii) std::copy(rad.begin(), rad.end(), radii);
        if (center_status) std::copy(st_c.begin(), st_c.end(), center_status);
        for (int p = 0; p < K; ++p) {
            if (st_c[p] < 0) { g_err = "centre LP did not converge for new region " + std::to_string(p); return GCSADMM_ERR_BAD_ARG; }
            if (!(rad[p] > 0.0)) { g_err = "new region " + std::to_string(p) + " has no interior"; return GCSADMM_ERR_BAD_ARG; }
        }

        // their boxes, failed sides opened
        LPRUN(for_dim(n, [&](auto N) {
            return launch_bounds<decltype(N)::value>(nx, P, K, nx.cen.get(), nx.lo.get(), nx.hi.get(), nx.st_b.get() + uP * 2 * un);
        }));
        hipLaunchKernelGGL(open_failed_sides_kernel, dim3(blocks_of((long)K * 2 * n)), dim3(TB), 0, 0, nx.st_b.get() + uP * 2 * un, n, K, nx.lo.get() + uP * un,
                           nx.hi.get() + uP * un);
        LPCHK(hipGetLastError());

        // sweep order of the new boxes (sorted on the host, as the resident ones were), ranks of all boxes, the merged sweep arrays
        std::vector<double> lo_new(uK * un), alo0(uK);
        LPCHK(to_host(lo_new.data(), nx.lo.get() + uP * un, uK * un));
        for (int p = 0; p < K; ++p) {
            alo0[p] = lo_new[(size_t)p * un];
            if (!(alo0[p] == alo0[p])) { g_err = "new box with a NaN lower bound"; return GCSADMM_ERR_BAD_ARG; }
        }
        std::vector<int> aorder(uK);
        sweep_order(alo0.data(), K, aorder.data());
        DevBuf<int> d_aorder, d_arank, d_inv, d_oldpos;
        DevBuf<double> aslo, ashi;
        LPCHK(d_aorder.put(aorder.data(), uK));
        LPCHK(d_arank.alloc(uK)); LPCHK(d_inv.alloc(uP + uK)); LPCHK(d_oldpos.alloc(uP + uK));
        LPCHK(aslo.alloc(uK * un)); LPCHK(ashi.alloc(uK * un));
        hipLaunchKernelGGL(sweep_gather_kernel, dim3(blocks_of(K)), dim3(TB), 0, 0, nx.lo.get() + uP * un, nx.hi.get() + uP * un, d_aorder.get(), n, K, aslo.get(),
                           ashi.get());
        const EditRanks ranks{P, K, old.slo.get(), aslo.get(), old.order.get(), d_aorder.get(), d_arank.get(), nx.order.get(), d_inv.get(),
                              d_oldpos.get()};
        hipLaunchKernelGGL(edit_rank_kernel, dim3(blocks_of(nx.P)), dim3(TB), 0, 0, ranks);
        hipLaunchKernelGGL(sweep_gather_kernel, dim3(blocks_of(nx.P)), dim3(TB), 0, 0, nx.lo.get(), nx.hi.get(), nx.order.get(), n, nx.P, nx.slo.get(), nx.shi.get());
        LPCHK(hipGetLastError());

        // cross sweep, count pass: the new boxes over all boxes behind them (F), the resident boxes over the new boxes behind them (B)
        CrossSide F{}, B{};
        F.S = SortedBoxes{K, aslo.get(), ashi.get(), d_aorder.get()}; F.T = SortedBoxes{nx.P, nx.slo.get(), nx.shi.get(), nx.order.get()};
        F.srank = d_arank.get(); F.chunks = edit_chunks(nx.P); F.cell0 = 0;
        B.S = SortedBoxes{P, old.slo.get(), old.shi.get(), old.order.get()}; B.T = F.S;
        B.trank = d_arank.get(); B.chunks = edit_chunks(K); B.cell0 = (long long)K * F.chunks;
        F.norder = B.norder = nx.order.get();
        const long long cells = B.cell0 + (long long)P * B.chunks;
        if (cells > INT32_MAX) { g_err = "more than 2^31 - 1 cells of the cross sweep: add fewer regions per call"; return GCSADMM_ERR_UNSUPPORTED; }
        DevBuf<int> d_cells;
        LPCHK(d_cells.alloc((size_t)cells));
        F.count = B.count = d_cells.get();
        auto cross = [&](bool fill) -> int {
            LPRUN(for_dim(n, [&](auto N) { return launch_cross<decltype(N)::value>(F, K, pad, fill); }));
            return for_dim(n, [&](auto N) { return launch_cross<decltype(N)::value>(B, P, pad, fill); });
        };
        LPRUN(cross(false));
        std::vector<int> cell_count((size_t)cells);
        std::vector<long long> cell_off((size_t)cells + 1);
        LPCHK(to_host(cell_count.data(), d_cells.get(), (size_t)cells));
        if (!edit_scan(cell_count.data(), cells, cell_off.data()) || cell_off[(size_t)cells] + oldp.T > (long long)INT32_MAX) {      // before anything is allocated
            g_err = "more than 2^31 - 1 candidate pairs"; return GCSADMM_ERR_UNSUPPORTED;
        }
        const long long Tn = cell_off[(size_t)cells], T = oldp.T + Tn;

        // fill pass, then the LPs of the new pairs, each from the centre of its first region
        DevBuf<long long> d_cell_off;
        DevBuf<int> rank_e, rank_l, npa, npb, nst;
        DevBuf<unsigned char> nflag;
        LPCHK(d_cell_off.put(cell_off.data(), cell_off.size()));
        LPCHK(rank_e.alloc((size_t)Tn)); LPCHK(rank_l.alloc((size_t)Tn)); LPCHK(npa.alloc((size_t)Tn)); LPCHK(npb.alloc((size_t)Tn));
        LPCHK(nst.alloc((size_t)Tn)); LPCHK(nflag.alloc((size_t)Tn));
        F.offset = B.offset = d_cell_off.get(); F.limit = B.limit = Tn;
        F.rank_e = B.rank_e = rank_e.get(); F.rank_l = B.rank_l = rank_l.get(); F.pair_a = B.pair_a = npa.get(); F.pair_b = B.pair_b = npb.get();
        if (Tn > 0) LPRUN(cross(true));
        LPRUN(for_dim(n, [&](auto N) {
            return launch_ball<decltype(N)::value>(nx, (long)Tn, npa.get(), npb.get(), nx.cen.get(), overlap_rows(nx.maxm), tol, 1, nullptr, nflag.get(), nst.get());
        }));
        unsigned long long decided[2];
        LPRUN(count_decisions(old, nflag.get(), nst.get(), (long)Tn, decided));

        // merge: counts by rank, scan, every pair to its place
        EditMerge m{};
        m.P = P; m.K = K; m.T_old = oldp.T; m.T_new = Tn; m.chunks_f = F.chunks; m.chunks_b = B.chunks; m.cell_off = d_cell_off.get();
        m.oldpos = d_oldpos.get(); m.inv = d_inv.get(); m.count_old = old.count.get(); m.offset_old = old.offset.get();
        m.pa_old = oldp.pa.get(); m.pb_old = oldp.pb.get(); m.st_old = oldp.st_o.get(); m.flag_old = oldp.flag.get();
        m.rank_e = rank_e.get(); m.rank_l = rank_l.get(); m.pa_new = npa.get(); m.pb_new = npb.get(); m.st_new = nst.get(); m.flag_new = nflag.get();
        m.count = nx.count.get();
        hipLaunchKernelGGL(merge_count_kernel, dim3(blocks_of(nx.P)), dim3(TB), 0, 0, m);
        LPCHK(hipGetLastError());
        std::vector<int> count((size_t)nx.P);
        std::vector<long long> offset((size_t)nx.P);
        LPCHK(to_host(count.data(), nx.count.get(), (size_t)nx.P));
        long long total = 0;
        if (!sweep_scan(count.data(), nx.P, offset.data(), &total) || total != T) { g_err = "the merged pair list does not add up"; return GCSADMM_ERR_HIP; }
        LPCHK(to_device(nx.offset.get(), offset.data(), offset.size()));
        LPRUN(alloc_buffers(nx, nxp, BUF_PAIRS, (size_t)T));
        m.offset = nx.offset.get(); m.pa = nxp.pa.get(); m.pb = nxp.pb.get(); m.st = nxp.st_o.get(); m.flag = nxp.flag.get();
        if (m.T_old > 0) hipLaunchKernelGGL(merge_move_old_kernel, dim3(blocks_of((long)m.T_old)), dim3(TB), 0, 0, m);
        if (Tn > 0) hipLaunchKernelGGL(merge_move_new_kernel, dim3(blocks_of((long)Tn)), dim3(TB), 0, 0, m);
        LPCHK(hipGetLastError());
        LPCHK(hipStreamSynchronize(nullptr));

        // the edited groups take the place of the resident ones (nothing here can fail)
        nxp.T = T;
        std::swap(s->reg, nx); std::swap(s->pairs, nxp);
        stage_finish(s->have, CALL_ADD_REGIONS);
        if (num_new_pairs) *num_new_pairs = Tn;
        if (num_overlapping) *num_overlapping = (int64_t)decided[0];
        if (num_undecided) *num_undecided = (int64_t)decided[1];
        return GCSADMM_OK;
    });
}

int gcsadmm_scene_remove_regions(gcsadmm_scene s, int R, const int *regions, int64_t *num_pairs_left)
{
    return scene_entry(s, [&]() -> int {
        if (R < 0 || (R > 0 && !regions)) { g_err = "negative number of regions or null index array"; return GCSADMM_ERR_BAD_ARG; }
        const SceneRegions &old = s->reg;
        const ScenePairs &oldp = s->pairs;
        const bool with_pairs = has(s->have, HAVE_PAIRS);
        const int n = old.n, P = old.P;
        const size_t un = (size_t)n, uP = (size_t)P;
        std::vector<int> newidx(uP);
        int Q = 0;
        if (!remove_renumber(P, R, regions, newidx.data(), &Q)) { g_err = "region index out of range or given twice"; return GCSADMM_ERR_BAD_ARG; }
        if (num_pairs_left) *num_pairs_left = with_pairs ? oldp.T : 0;
        if (R == 0) return GCSADMM_OK;
        const size_t uQ = (size_t)Q;
        SceneRegions nx;
        ScenePairs nxp;
        nx.n = n; nx.P = Q;
        nx.h_ptr.assign(1, 0);
        for (int p = 0; p < P; ++p) {
            if (newidx[p] < 0) continue;
            const int m = old.h_ptr[(size_t)p + 1] - old.h_ptr[p];
            nx.maxm = std::max(nx.maxm, m);
            nx.h_ptr.push_back(nx.h_ptr.back() + m);
        }
        const size_t rows = (size_t)nx.h_ptr.back();

        // the polytopes and the per-region results: row p to row newidx[p]
        DevBuf<int> d_newidx;
        LPCHK(d_newidx.put(newidx.data(), uP));
        LPCHK(nx.ptr.put(nx.h_ptr.data(), nx.h_ptr.size()));
        LPCHK(nx.A.alloc(rows * un)); LPCHK(nx.b.alloc(rows)); LPCHK(nx.nrm.alloc(rows));
        LPRUN(alloc_buffers(nx, nxp, BUF_CEN | BUF_CENTRE_LP | BUF_BOXES | BUF_RESIDENT));
        const dim3 grid(blocks_of(P)), block(TB);
        hipLaunchKernelGGL(compact_polys_kernel, grid, block, 0, 0, old.ptr.get(), nx.ptr.get(), d_newidx.get(), n, P, old.A.get(), old.b.get(), old.nrm.get(),
                           nx.A.get(), nx.b.get(), nx.nrm.get());
        auto compact = [&](auto &src, auto &dst, int width) {
            using V = std::remove_pointer_t<decltype(src.get())>;
            hipLaunchKernelGGL(compact_rows_kernel<V>, grid, block, 0, 0, (const V *)src.get(), dst.get(), (const int *)d_newidx.get(), width, P);
        };
        compact(old.w, nx.w, n + 1); compact(old.cen, nx.cen, n); compact(old.rad, nx.rad, 1); compact(old.st_c, nx.st_c, 1);
        compact(old.lo, nx.lo, n); compact(old.hi, nx.hi, n); compact(old.st_b, nx.st_b, 2 * n);
        LPCHK(hipGetLastError());

        // the pair list: the segments of the old sweep order, without the removed boxes and their pairs
        long long T = 0;
        DevBuf<int> d_kept;
        DevBuf<long long> d_dst;
        if (with_pairs) {
            LPCHK(d_kept.alloc(uP));
            EditRemove e{};
            e.P = P; e.newidx = d_newidx.get(); e.order = old.order.get(); e.count_old = old.count.get(); e.offset_old = old.offset.get();
            e.pa_old = oldp.pa.get(); e.pb_old = oldp.pb.get(); e.st_old = oldp.st_o.get(); e.flag_old = oldp.flag.get(); e.kept = d_kept.get();
            hipLaunchKernelGGL(remove_segment_kernel<false>, grid, block, 0, 0, e);
            LPCHK(hipGetLastError());
            std::vector<int> kept(uP), order(uP), new_order, new_count;
            std::vector<long long> dst(uP, 0), new_offset;
            LPCHK(to_host(kept.data(), d_kept.get(), uP)); LPCHK(to_host(order.data(), old.order.get(), uP));
            for (int i = 0; i < P; ++i) {
                dst[i] = T;
                if (newidx[order[i]] < 0) continue;
                new_order.push_back(newidx[order[i]]); new_count.push_back(kept[i]); new_offset.push_back(T);
                T += kept[i];
            }
            LPCHK(to_device(nx.order.get(), new_order.data(), uQ)); LPCHK(to_device(nx.count.get(), new_count.data(), uQ));
            LPCHK(to_device(nx.offset.get(), new_offset.data(), uQ));
            LPCHK(d_dst.put(dst.data(), uP));
            LPRUN(alloc_buffers(nx, nxp, BUF_PAIRS, (size_t)T));
            e.dst = d_dst.get(); e.pa = nxp.pa.get(); e.pb = nxp.pb.get(); e.st = nxp.st_o.get(); e.flag = nxp.flag.get();
            hipLaunchKernelGGL(remove_segment_kernel<true>, grid, block, 0, 0, e);
            if (Q > 0)
                hipLaunchKernelGGL(sweep_gather_kernel, dim3(blocks_of(Q)), block, 0, 0, nx.lo.get(), nx.hi.get(), nx.order.get(), n, Q, nx.slo.get(), nx.shi.get());
            LPCHK(hipGetLastError());
        }
        LPCHK(hipStreamSynchronize(nullptr));

        // the edited groups take the place of the resident ones (nothing here can fail); a scene without pairs keeps having none
        nxp.T = T;
        std::swap(s->reg, nx);
        if (with_pairs) std::swap(s->pairs, nxp);
        stage_finish(s->have, CALL_REMOVE_REGIONS);
        if (num_pairs_left) *num_pairs_left = T;
        return GCSADMM_OK;
    });
}

// ---- the region graph of a decided scene, and the query graphs of a batch from it (query_graph_core.h) ----
int gcsadmm_scene_build_region_graph(gcsadmm_scene s, const unsigned char *overlap, int64_t *num_edges)
{
    return scene_entry(s, [&]() -> int {
        NEED(s, CALL_BUILD_GRAPH);
        const ScenePairs &pr = s->pairs;
        const int P = s->reg.P;
        const long long T = pr.T;
        DevBuf<unsigned char> d_flag;
        SceneGraph nx;
        DevBuf<int> d_count, unsorted;
        if (overlap) LPCHK(d_flag.put(overlap, (size_t)T));
        LPCHK(d_count.upload(nullptr, (size_t)P));
        RegionBuild g{};
        g.P = P; g.T = T; g.pa = pr.pa.get(); g.pb = pr.pb.get(); g.flag = overlap ? d_flag.get() : pr.flag.get(); g.count = d_count.get();
        if (T > 0) hipLaunchKernelGGL(region_count_kernel, dim3(blocks_of((long)T)), dim3(TB), 0, 0, g);
        LPCHK(hipGetLastError());
        std::vector<int> count((size_t)P);
        std::vector<long long> row_ptr((size_t)P + 1);
        LPCHK(to_host(count.data(), d_count.get(), (size_t)P));
        if (!region_scan(count.data(), P, row_ptr.data())) {      // before the graph is allocated
            g_err = "too many region edges: a query graph's incidences would not fit 32-bit indices"; return GCSADMM_ERR_UNSUPPORTED;
        }
        const long long E = row_ptr[(size_t)P];
        LPCHK(nx.row_ptr.put(row_ptr.data(), row_ptr.size()));
        LPCHK(unsorted.alloc((size_t)E)); LPCHK(nx.tail.alloc((size_t)E)); LPCHK(nx.head.alloc((size_t)E)); LPCHK(nx.rev.alloc((size_t)E));
        LPCHK(hipMemset(d_count.get(), 0, sizeof(int) * std::max<size_t>((size_t)P, 1)));
        g.row_ptr = nx.row_ptr.get(); g.unsorted = unsorted.get(); g.tail = nx.tail.get(); g.head = nx.head.get(); g.rev = nx.rev.get();
        if (E > 0) {
            hipLaunchKernelGGL(region_scatter_kernel, dim3(blocks_of((long)T)), dim3(TB), 0, 0, g);
            hipLaunchKernelGGL(region_place_kernel, dim3(blocks_of((long)E)), dim3(TB), 0, 0, g, E);
            hipLaunchKernelGGL(region_reverse_kernel, dim3(blocks_of((long)E)), dim3(TB), 0, 0, g, E);
        }
        LPCHK(hipGetLastError());
        LPCHK(hipStreamSynchronize(nullptr));
        nx.edges = E;
        std::swap(s->graph, nx);
        stage_finish(s->have, CALL_BUILD_GRAPH);
        if (num_edges) *num_edges = E;
        return GCSADMM_OK;
    });
}

int gcsadmm_scene_read_region_graph(gcsadmm_scene s, int64_t *row_ptr, int *edge_tail, int *edge_head, int *reverse)
{
    return scene_entry(s, [&]() -> int {
        NEED(s, CALL_READ_GRAPH);
        static_assert(sizeof(int64_t) == sizeof(long long), "row_ptr is kept as long long");
        LPCHK(to_host((long long *)row_ptr, s->graph.row_ptr));
        LPCHK(to_host(edge_tail, s->graph.tail)); LPCHK(to_host(edge_head, s->graph.head)); LPCHK(to_host(reverse, s->graph.rev));
        return GCSADMM_OK;
    });
}

int gcsadmm_scene_query_graphs(gcsadmm_scene s, int B, const int64_t *term_ptr, const int *term_region, const unsigned char *st_adjacent,
                               int chunk_queries, const int64_t *edge_off, int *edge_tail, int *edge_head, int *inc_ptr, int *inc_edge, int *inc_out,
                               int *edge_inc_tail, int *edge_inc_head)
{
    return scene_entry(s, [&]() -> int {
        static_assert(QUERY_BAD_ARG == GCSADMM_ERR_BAD_ARG && QUERY_UNSUPPORTED == GCSADMM_ERR_UNSUPPORTED && QUERY_OK == GCSADMM_OK, "query_check returns the ABI's codes");
        NEED(s, CALL_QUERY_GRAPHS);
        const SceneGraph &rg = s->graph;
        QueryScratch &qg = s->qg;
        const int P = s->reg.P;
        const QueryBatch host{B, (const long long *)term_ptr, term_region, st_adjacent, (const long long *)edge_off};
        long long max_items = 0;
        LPRUN(query_check(P, rg.edges, host, chunk_queries, g_err, &max_items));
        if (B == 0) return GCSADMM_OK;
        if (!edge_tail || !edge_head || !inc_ptr || !inc_edge || !inc_out || !edge_inc_tail || !edge_inc_head) { g_err = "null output array"; return GCSADMM_ERR_BAD_ARG; }
        const size_t points = 2 * (size_t)B, hits = (size_t)host.term_ptr[points], V1 = (size_t)P + 3;
        LPCHK(qg.term_ptr.reserve(points + 1)); LPCHK(qg.term_region.reserve(hits)); LPCHK(qg.st.reserve((size_t)B)); LPCHK(qg.edge_off.reserve((size_t)B + 1));
        LPCHK(to_device(qg.term_ptr.get(), host.term_ptr, points + 1));
        LPCHK(to_device(qg.term_region.get(), term_region, hits));
        LPCHK(to_device(qg.st.get(), st_adjacent, (size_t)B));
        LPCHK(to_device(qg.edge_off.get(), host.edge_off, (size_t)B + 1));
        QueryGraphArgs a{};
        a.g = RegionGraph{P, rg.edges, rg.row_ptr.get(), rg.tail.get(), rg.head.get(), rg.rev.get()};
        a.q = QueryBatch{B, qg.term_ptr.get(), qg.term_region.get(), qg.st.get(), qg.edge_off.get()};
        a.items = max_items;
        const int chunk = query_chunk(P, rg.edges, chunk_queries);
        for (int first = 0; first < B; first += chunk) {
            const int count = std::min(chunk, B - first);
            const size_t at = (size_t)host.edge_off[first], E = (size_t)(host.edge_off[first + count] - host.edge_off[first]);
            LPCHK(qg.edge_tail.reserve(E)); LPCHK(qg.edge_head.reserve(E)); LPCHK(qg.inc_ptr.reserve((size_t)count * V1));
            LPCHK(qg.inc_edge.reserve(2 * E)); LPCHK(qg.inc_out.reserve(2 * E)); LPCHK(qg.edge_inc_tail.reserve(E)); LPCHK(qg.edge_inc_head.reserve(E));
            a.out = QueryArrays{qg.edge_tail.get(), qg.edge_head.get(), qg.inc_ptr.get(), qg.inc_edge.get(), qg.inc_out.get(),
                                qg.edge_inc_tail.get(), qg.edge_inc_head.get()};
            a.first = first;
            hipLaunchKernelGGL(query_graph_kernel, dim3((unsigned)((max_items + 255) / 256), (unsigned)count), dim3(256), 0, 0, a);
            LPCHK(hipGetLastError());
            LPCHK(to_host(edge_tail + at, a.out.edge_tail, E)); LPCHK(to_host(edge_head + at, a.out.edge_head, E));
            LPCHK(to_host(inc_ptr + (size_t)first * V1, a.out.inc_ptr, (size_t)count * V1));
            LPCHK(to_host(inc_edge + 2 * at, a.out.inc_edge, 2 * E)); LPCHK(to_host(inc_out + 2 * at, a.out.inc_out, 2 * E));
            LPCHK(to_host(edge_inc_tail + at, a.out.edge_inc_tail, E)); LPCHK(to_host(edge_inc_head + at, a.out.edge_inc_head, E));
        }
        LPCHK(hipStreamSynchronize(nullptr));
        return GCSADMM_OK;
    });
}

// ---- the informed region set of every query of a batch (informed_core.h); like restrict_paths outside the table of scene_stage.h ----
// the weights of the region graph's edges: made once per graph, by the first path call on it (region_paths or region_paths_sets)
static int region_weights(const SceneRegions &r, SceneGraph &rg)
{
    if (rg.w) return GCSADMM_OK;
    LPCHK(rg.w.alloc((size_t)rg.edges));
    if (rg.edges > 0)
        hipLaunchKernelGGL(region_weight_kernel, dim3(blocks_of((long)rg.edges)), dim3(TB), 0, 0, r.cen.get(), r.n, rg.tail.get(), rg.head.get(), rg.edges, rg.w.get());
    LPCHK(hipGetLastError());
    return GCSADMM_OK;
}
int gcsadmm_scene_region_paths(gcsadmm_scene s, int num_queries, const double *points, const int64_t *term_ptr, const int *term_region,
                               int max_len, int *path_region, int *path_len, double *path_cost, int *status)
{
    return scene_entry(s, [&]() -> int {
        for (const NeedRule &rule : {NEED_FRESH_GRAPH, NEED_CENTERS})
            if (!has(s->have, rule.flags)) { g_err = rule.refusal; return GCSADMM_ERR_BAD_ARG; }
        const SceneRegions &r = s->reg;
        SceneGraph &rg = s->graph;
        InformedScratch &q = s->inf;
        const int B = num_queries, P = r.P, n = r.n;
        LPRUN(informed_check_paths(P, n, B, points, (const long long *)term_ptr, term_region, max_len, g_err));
        if (B == 0) return GCSADMM_OK;
        if (!path_region || !path_len || !path_cost || !status) { g_err = "null output array"; return GCSADMM_ERR_BAD_ARG; }
        if ((long long)B * max_len > (long long)INT32_MAX) { g_err = "num_queries * max_len above 2^31 - 1"; return GCSADMM_ERR_UNSUPPORTED; }
        LPRUN(region_weights(r, rg));
        const size_t coords = 2 * (size_t)B * n, hits = (size_t)term_ptr[2 * (size_t)B], cells = (size_t)B * max_len;
        const int chunk = informed_chunk(P);
        LPCHK(q.points.reserve(coords)); LPCHK(q.term_ptr.reserve(2 * (size_t)B + 1)); LPCHK(q.term_region.reserve(hits));
        LPCHK(q.d.reserve((size_t)std::min(chunk, B) * P));
        LPCHK(q.path_region.reserve(cells)); LPCHK(q.path_len.reserve((size_t)B)); LPCHK(q.status.reserve((size_t)B)); LPCHK(q.cost.reserve((size_t)B));
        LPCHK(to_device(q.points.get(), points, coords));
        LPCHK(to_device(q.term_ptr.get(), (const long long *)term_ptr, 2 * (size_t)B + 1));
        if (hits > 0) LPCHK(to_device(q.term_region.get(), term_region, hits));      // (no hit at all: term_region may be null; the buffer is there)
        LPCHK(hipMemset(q.path_region.get(), 0xff, sizeof(int) * cells));      // entries beyond a path's length: -1
        PathArgs a{};
        a.g = PathGraph{P, n, rg.row_ptr.get(), rg.head.get(), rg.w.get(), r.cen.get()};
        a.points = q.points.get(); a.term_ptr = q.term_ptr.get(); a.term_region = q.term_region.get();
        a.B = B; a.max_len = max_len; a.d = q.d.get();
        a.path_region = q.path_region.get(); a.path_len = q.path_len.get(); a.status = q.status.get(); a.path_cost = q.cost.get();
        for (int first = 0; first < B; first += chunk) {      // (a chunk's launch follows the one before on the stream: d is theirs in turn)
            a.first = first;
            hipLaunchKernelGGL(region_path_kernel, dim3((unsigned)std::min(chunk, B - first)), dim3(PATH_THREADS), 0, 0, a);
            LPCHK(hipGetLastError());
        }
        LPCHK(to_host(path_region, q.path_region.get(), cells)); LPCHK(to_host(path_len, q.path_len.get(), (size_t)B));
        LPCHK(to_host(path_cost, q.cost.get(), (size_t)B)); LPCHK(to_host(status, q.status.get(), (size_t)B));
        LPCHK(hipStreamSynchronize(nullptr));
        return GCSADMM_OK;
    });
}

int gcsadmm_scene_informed_regions(gcsadmm_scene s, int num_queries, const double *points, const double *bound, double pad,
                                   unsigned char *keep, int64_t *num_kept)
{
    return scene_entry(s, [&]() -> int {
        if (!has(s->have, NEED_BOXES.flags)) { g_err = NEED_BOXES.refusal; return GCSADMM_ERR_BAD_ARG; }
        const SceneRegions &r = s->reg;
        InformedScratch &q = s->inf;
        const int B = num_queries, P = r.P, n = r.n;
        LPRUN(informed_check_keep(n, B, points, bound, pad, g_err));
        if (B == 0) return GCSADMM_OK;
        if (!keep) { g_err = "null output array"; return GCSADMM_ERR_BAD_ARG; }
        const size_t coords = 2 * (size_t)B * n, cells = (size_t)B * P;
        LPCHK(q.points.reserve(coords)); LPCHK(q.bound.reserve((size_t)B)); LPCHK(q.keep.reserve(cells));
        LPCHK(to_device(q.points.get(), points, coords)); LPCHK(to_device(q.bound.get(), bound, (size_t)B));
        KeepArgs a{P, n, B, 0, r.lo.get(), r.hi.get(), q.points.get(), q.bound.get(), pad, q.keep.get()};
        for (int first = 0; first < B && P > 0; first += QUERY_CHUNK_MAX) {      // grid.y
            a.first = first;
            hipLaunchKernelGGL(informed_keep_kernel, dim3(blocks_of(P), (unsigned)std::min(QUERY_CHUNK_MAX, B - first)), dim3(TB), 0, 0, a);
            LPCHK(hipGetLastError());
        }
        LPCHK(to_host(keep, q.keep.get(), cells));
        LPCHK(hipStreamSynchronize(nullptr));
        if (num_kept)
            for (int i = 0; i < B; ++i) {
                int64_t kept = 0;
                for (int p = 0; p < P; ++p) kept += keep[(size_t)i * P + p];
                num_kept[i] = kept;
            }
        return GCSADMM_OK;
    });
}

// ---- the same for start and goal sets (informed_set_core.h): the two calls above with boxes in the place of the points ----
int gcsadmm_scene_region_paths_sets(gcsadmm_scene s, int num_queries, const double *lo, const double *hi, const int64_t *term_ptr,
                                    const int *term_region, int max_len, int *path_region, int *path_len, double *path_cost, int *status)
{
    return scene_entry(s, [&]() -> int {
        for (const NeedRule &rule : {NEED_FRESH_GRAPH, NEED_CENTERS})
            if (!has(s->have, rule.flags)) { g_err = rule.refusal; return GCSADMM_ERR_BAD_ARG; }
        const SceneRegions &r = s->reg;
        SceneGraph &rg = s->graph;
        InformedScratch &q = s->inf;
        const int B = num_queries, P = r.P, n = r.n;
        LPRUN(set_check_paths(P, n, B, lo, hi, (const long long *)term_ptr, term_region, max_len, g_err));
        if (B == 0) return GCSADMM_OK;
        if (!path_region || !path_len || !path_cost || !status) { g_err = "null output array"; return GCSADMM_ERR_BAD_ARG; }
        if ((long long)B * max_len > (long long)INT32_MAX) { g_err = "num_queries * max_len above 2^31 - 1"; return GCSADMM_ERR_UNSUPPORTED; }
        LPRUN(region_weights(r, rg));
        const size_t coords = 2 * (size_t)B * n, hits = (size_t)term_ptr[2 * (size_t)B], cells = (size_t)B * max_len;
        const int chunk = informed_chunk(P);
        LPCHK(q.points.reserve(2 * coords)); LPCHK(q.term_ptr.reserve(2 * (size_t)B + 1)); LPCHK(q.term_region.reserve(hits));      // points: lo, then hi
        LPCHK(q.d.reserve((size_t)std::min(chunk, B) * P));
        LPCHK(q.path_region.reserve(cells)); LPCHK(q.path_len.reserve((size_t)B)); LPCHK(q.status.reserve((size_t)B)); LPCHK(q.cost.reserve((size_t)B));
        LPCHK(to_device(q.points.get(), lo, coords)); LPCHK(to_device(q.points.get() + coords, hi, coords));
        LPCHK(to_device(q.term_ptr.get(), (const long long *)term_ptr, 2 * (size_t)B + 1));
        if (hits > 0) LPCHK(to_device(q.term_region.get(), term_region, hits));
        LPCHK(hipMemset(q.path_region.get(), 0xff, sizeof(int) * cells));      // entries beyond a path's length: -1
        SetPathArgs a{};
        a.g = PathGraph{P, n, rg.row_ptr.get(), rg.head.get(), rg.w.get(), r.cen.get()};
        a.lo = q.points.get(); a.hi = q.points.get() + coords; a.term_ptr = q.term_ptr.get(); a.term_region = q.term_region.get();
        a.B = B; a.max_len = max_len; a.d = q.d.get();
        a.path_region = q.path_region.get(); a.path_len = q.path_len.get(); a.status = q.status.get(); a.path_cost = q.cost.get();
        for (int first = 0; first < B; first += chunk) {
            a.first = first;
            hipLaunchKernelGGL(terminal_set_path_kernel, dim3((unsigned)std::min(chunk, B - first)), dim3(PATH_THREADS), 0, 0, a);
            LPCHK(hipGetLastError());
        }
        LPCHK(to_host(path_region, q.path_region.get(), cells)); LPCHK(to_host(path_len, q.path_len.get(), (size_t)B));
        LPCHK(to_host(path_cost, q.cost.get(), (size_t)B)); LPCHK(to_host(status, q.status.get(), (size_t)B));
        LPCHK(hipStreamSynchronize(nullptr));
        return GCSADMM_OK;
    });
}

int gcsadmm_scene_informed_regions_sets(gcsadmm_scene s, int num_queries, const double *lo, const double *hi, const double *bound, double pad,
                                        unsigned char *keep, int64_t *num_kept)
{
    return scene_entry(s, [&]() -> int {
        if (!has(s->have, NEED_BOXES.flags)) { g_err = NEED_BOXES.refusal; return GCSADMM_ERR_BAD_ARG; }
        const SceneRegions &r = s->reg;
        InformedScratch &q = s->inf;
        const int B = num_queries, P = r.P, n = r.n;
        LPRUN(set_check_keep(n, B, lo, hi, bound, pad, g_err));
        if (B == 0) return GCSADMM_OK;
        if (!keep) { g_err = "null output array"; return GCSADMM_ERR_BAD_ARG; }
        const size_t coords = 2 * (size_t)B * n, cells = (size_t)B * P;
        LPCHK(q.points.reserve(2 * coords)); LPCHK(q.bound.reserve((size_t)B)); LPCHK(q.keep.reserve(cells));
        LPCHK(to_device(q.points.get(), lo, coords)); LPCHK(to_device(q.points.get() + coords, hi, coords));
        LPCHK(to_device(q.bound.get(), bound, (size_t)B));
        SetKeepArgs a{P, n, B, 0, r.lo.get(), r.hi.get(), q.points.get(), q.points.get() + coords, q.bound.get(), pad, q.keep.get()};
        for (int first = 0; first < B && P > 0; first += QUERY_CHUNK_MAX) {      // grid.y
            a.first = first;
            hipLaunchKernelGGL(terminal_set_keep_kernel, dim3(blocks_of(P), (unsigned)std::min(QUERY_CHUNK_MAX, B - first)), dim3(TB), 0, 0, a);
            LPCHK(hipGetLastError());
        }
        LPCHK(to_host(keep, q.keep.get(), cells));
        LPCHK(hipStreamSynchronize(nullptr));
        if (num_kept)
            for (int i = 0; i < B; ++i) {
                int64_t kept = 0;
                for (int p = 0; p < P; ++p) kept += keep[(size_t)i * P + p];
                num_kept[i] = kept;
            }
        return GCSADMM_OK;
    });
}

// ---- the query graphs of a batch on each query's kept regions (induced_graph_core.h); like region_paths outside the table of scene_stage.h ----
int gcsadmm_scene_induced_sizes(gcsadmm_scene s, int num_queries, const unsigned char *keep, const int64_t *term_ptr, const int *term_region,
                                const unsigned char *st_adjacent, int *num_kept, int64_t *num_edges)
{
    return scene_entry(s, [&]() -> int {
        const InducedBatch host{num_queries, keep, (const long long *)term_ptr, term_region, st_adjacent};
        if (num_queries > 0 && (!num_kept || !num_edges)) { g_err = "null output array"; return GCSADMM_ERR_BAD_ARG; }
        std::vector<int> sizes;
        int chunk = 0;
        LPRUN(induced_counts(*s, host, 0, chunk, sizes));
        const QueryBatch b{host.B, host.term_ptr, host.term_region, host.st, nullptr};
        for (int i = 0; i < num_queries; ++i) {
            const QueryTerms t = query_terms(b, i);
            num_kept[i] = sizes[(size_t)INDUCED_SIZES * i];
            num_edges[i] = query_edges(sizes[(size_t)INDUCED_SIZES * i + 1], t.a, t.b, t.c);
        }
        return GCSADMM_OK;
    });
}

int gcsadmm_scene_induced_query_graphs(gcsadmm_scene s, int num_queries, const unsigned char *keep, const int64_t *term_ptr, const int *term_region,
                                       const unsigned char *st_adjacent, int chunk_queries, const int64_t *vertex_off, const int64_t *edge_off,
                                       int *edge_tail, int *edge_head, int *inc_ptr, int *inc_edge, int *inc_out, int *edge_inc_tail, int *edge_inc_head)
{
    return scene_entry(s, [&]() -> int {
        const InducedBatch host{num_queries, keep, (const long long *)term_ptr, term_region, st_adjacent};
        const int B = num_queries;
        if (B > 0 && (!vertex_off || !edge_off || !edge_tail || !edge_head || !inc_ptr || !inc_edge || !inc_out || !edge_inc_tail || !edge_inc_head)) {
            g_err = "null vertex_off, edge_off or output array"; return GCSADMM_ERR_BAD_ARG;
        }
        std::vector<int> sizes, again;
        int chunk = 0;
        LPRUN(induced_counts(*s, host, chunk_queries, chunk, sizes));
        if (B == 0) return GCSADMM_OK;
        const long long *v_off = (const long long *)vertex_off, *e_off = (const long long *)edge_off;
        LPRUN(induced_check_offsets(host, sizes.data(), v_off, e_off, g_err));      // nothing of the caller's is written before this
        InducedScratch &w = s->ig;
        LPCHK(w.vertex_off.reserve((size_t)B + 1)); LPCHK(w.edge_off.reserve((size_t)B + 1));
        LPCHK(to_device(w.vertex_off.get(), v_off, (size_t)B + 1)); LPCHK(to_device(w.edge_off.get(), e_off, (size_t)B + 1));
        const QueryArrays out{edge_tail, edge_head, inc_ptr, inc_edge, inc_out, edge_inc_tail, edge_inc_head};
        again.resize((size_t)INDUCED_SIZES * std::min(chunk, B));
        for (int first = 0; first < B; first += chunk) {
            const int count = std::min(chunk, B - first);
            if (chunk < B) LPRUN(induced_count(*s, host, first, count, again.data()));      // (several chunks: the count arrays are the last one's)
            LPRUN(induced_write(*s, host, first, count, sizes.data() + (size_t)INDUCED_SIZES * first, v_off, e_off, out));
        }
        LPCHK(hipStreamSynchronize(nullptr));
        return GCSADMM_OK;
    });
}

} // extern "C"
