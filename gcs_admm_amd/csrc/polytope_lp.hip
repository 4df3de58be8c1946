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
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdio>
#include <new>
#include <string>
#include <vector>

#include "gcsadmm.h"

#include "polytope_lp_core.h"
#include "box_sweep_core.h"

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
__global__ __launch_bounds__(WAVE) void bounds_kernel(Polys S, const double *centers, int maxm, double *lo, double *hi, int *out_status)
{
    extern __shared__ double smem[];
    double *lam = smem, *dlam = smem + (size_t)maxm * WAVE;
    const int t = blockIdx.x * WAVE + threadIdx.x, lane = threadIdx.x;
    if (t >= S.P * 2 * N) return;
    const int p = t / (2 * N), j = t % (2 * N), k = j >> 1, upper = j & 1;
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

static std::string g_err;

// the entry points switch to the requested device (upload_scene) and hand the caller's current device back on return
struct RestoreDevice {
    int prev = -1;
    RestoreDevice() { if (hipGetDevice(&prev) != hipSuccess) prev = -1; }
    ~RestoreDevice()
    {
        int cur = -1;
        if (prev >= 0 && hipGetDevice(&cur) == hipSuccess && cur != prev) (void)hipSetDevice(prev);
    }
};

struct DevBuf {
    void *p = nullptr;
    DevBuf() = default;
    DevBuf(const DevBuf &) = delete;
    DevBuf &operator=(const DevBuf &) = delete;
    ~DevBuf() { release(); }
    hipError_t alloc(size_t bytes) { release(); return hipMalloc(&p, bytes ? bytes : 8); }
    void release() { if (p) (void)hipFree(p); p = nullptr; }
    template <class T> T *as() { return (T *)p; }
};

struct Scene {
    DevBuf ptr, A, b, nrm;
    Polys S;
    int maxm = 0;
};

static int upload_scene(Scene &sc, int n, int P, const int *poly_ptr, const double *A, const double *b, int device)
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
        sc.maxm = std::max(sc.maxm, m);
    }
    const int rows = poly_ptr[P];
    std::vector<double> nrm((size_t)rows);
    for (int r = 0; r < rows; ++r) {
        double s = 0;
        for (int k = 0; k < n; ++k) s += A[(size_t)r * n + k] * A[(size_t)r * n + k];
        if (!(s > 0.0)) { g_err = "zero facet normal"; return GCSADMM_ERR_BAD_ARG; }
        nrm[r] = std::sqrt(s);
    }
    hipError_t e;
#define CK(x) if ((e = (x)) != hipSuccess) { g_err = std::string(#x) + ": " + hipGetErrorString(e); return GCSADMM_ERR_HIP; }
    CK(hipSetDevice(device));
    CK(sc.ptr.alloc(sizeof(int) * (P + 1))); CK(sc.A.alloc(sizeof(double) * rows * n));
    CK(sc.b.alloc(sizeof(double) * rows)); CK(sc.nrm.alloc(sizeof(double) * rows));
    CK(hipMemcpy(sc.ptr.p, poly_ptr, sizeof(int) * (P + 1), hipMemcpyHostToDevice));
    CK(hipMemcpy(sc.A.p, A, sizeof(double) * rows * n, hipMemcpyHostToDevice));
    CK(hipMemcpy(sc.b.p, b, sizeof(double) * rows, hipMemcpyHostToDevice));
    CK(hipMemcpy(sc.nrm.p, nrm.data(), sizeof(double) * rows, hipMemcpyHostToDevice));
    sc.S = Polys{n, P, sc.ptr.as<int>(), sc.A.as<double>(), sc.b.as<double>(), sc.nrm.as<double>()};
    return GCSADMM_OK;
}

template <int N>
static int launch_ball(const Scene &sc, long count, const int *d_pa, const int *d_pb, const double *d_x0, int rows_max,
                       double tol, int early, double *d_w, unsigned char *d_flag, int *d_status)
{
    const size_t lds = lds_bytes(rows_max);
    if (lds > LDS_MAX_BYTES) { g_err = "too many facet rows per LP for LDS"; return GCSADMM_ERR_UNSUPPORTED; }
    hipError_t e;
    CK(hipFuncSetAttribute((const void *)ball_kernel<N>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    if (count > 0)
        hipLaunchKernelGGL(ball_kernel<N>, dim3((unsigned)((count + WAVE - 1) / WAVE)), dim3(WAVE), lds, 0, sc.S, (int)count, d_pa, d_pb,
                           d_x0, rows_max, tol, early, d_w, d_flag, d_status);
    CK(hipGetLastError());
    return GCSADMM_OK;
}
template <int N>
static int launch_bounds(const Scene &sc, const double *d_centers, double *d_lo, double *d_hi, int *d_status)
{
    const int rows_max = bounds_rows(sc.maxm, N);
    const size_t lds = lds_bytes(rows_max);
    if (lds > LDS_MAX_BYTES) { g_err = "too many facet rows per LP for LDS"; return GCSADMM_ERR_UNSUPPORTED; }
    hipError_t e;
    CK(hipFuncSetAttribute((const void *)bounds_kernel<N>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    const long count = (long)sc.S.P * 2 * N;
    if (count > 0)
        hipLaunchKernelGGL(bounds_kernel<N>, dim3((unsigned)((count + WAVE - 1) / WAVE)), dim3(WAVE), lds, 0, sc.S, d_centers, rows_max, d_lo, d_hi, d_status);
    CK(hipGetLastError());
    return GCSADMM_OK;
}

#define DISPATCH_N(n, CALL)                                                                          \
    switch (n) {                                                                                       \
    case 1: { constexpr int NN = 1; rc = CALL; } break;                                                \
    case 2: { constexpr int NN = 2; rc = CALL; } break;                                                \
    case 3: { constexpr int NN = 3; rc = CALL; } break;                                                \
    case 4: { constexpr int NN = 4; rc = CALL; } break;                                                \
    case 5: { constexpr int NN = 5; rc = CALL; } break;                                                \
    case 6: { constexpr int NN = 6; rc = CALL; } break;                                                \
    case 7: { constexpr int NN = 7; rc = CALL; } break;                                                \
    default: { constexpr int NN = 8; rc = CALL; } break;                                               \
    }

} // namespace gcsadmm_lp

using namespace gcsadmm_lp;

// The resident scene: everything graph construction computes stays in these buffers until gcsadmm_scene_read_pairs.
struct gcsadmm_scene_s {
    Scene sc;
    int n = 0, P = 0, device = 0;
    DevBuf w, cen, rad, st_c;                          // centre LPs: (x, r) records, centres [P][n], radii, statuses
    DevBuf lo, hi, st_b;                               // boxes [P][n] and the statuses of their LPs [P][n][2]
    DevBuf lo0, order, slo, shi, count, offset;        // sweep: first lower bounds, sort order, sorted boxes [n][P], counts, offsets
    DevBuf pa, pb, flag, st_o, counts;                 // pair list with the narrow phase's flags and statuses, and the two counts of them
    long long T = 0;
    bool have_centers = false, have_boxes = false, have_pairs = false, have_overlaps = false;
};

namespace {

constexpr int TB = 256;      // threads per block of the element-wise helpers
inline unsigned blocks_of(long count) { return (unsigned)((count + TB - 1) / TB); }

template <int N>
int launch_sweep(gcsadmm_scene_s *s, bool fill, double pad)
{
    const SortedBoxes B{s->P, s->slo.as<double>(), s->shi.as<double>(), s->order.as<int>()};
    hipError_t e;
    if (s->P > 0) {
        if (fill)
            hipLaunchKernelGGL((sweep_kernel<N, true>), dim3((unsigned)s->P), dim3(SWEEP_WAVE), 0, 0, B, pad, nullptr,
                               s->offset.as<long long>(), s->pa.as<int>(), s->pb.as<int>());
        else
            hipLaunchKernelGGL((sweep_kernel<N, false>), dim3((unsigned)s->P), dim3(SWEEP_WAVE), 0, 0, B, pad, s->count.as<int>(), nullptr,
                               nullptr, nullptr);
    }
    CK(hipGetLastError());
    return GCSADMM_OK;
}

// entry of every scene call: the handle's device for the call, the caller's back on return (RestoreDevice in the caller's frame)
int enter_scene(gcsadmm_scene_s *s)
{
    if (!s) { g_err = "null scene"; return GCSADMM_ERR_BAD_ARG; }
    hipError_t e;
    CK(hipSetDevice(s->device));
    return GCSADMM_OK;
}

} // namespace

extern "C" {

const char *gcsadmm_polytope_last_error(void) { return g_err.c_str(); }

int gcsadmm_polytope_centers(int n, int num_polytopes, const int *poly_ptr, const double *poly_A, const double *poly_b,
                             int device, double *centers, double *radii, int *status)
{
    RestoreDevice restore_device_;
    if (!centers) { g_err = "null output"; return GCSADMM_ERR_BAD_ARG; }
    Scene sc;
    int rc = upload_scene(sc, n, num_polytopes, poly_ptr, poly_A, poly_b, device);
    if (rc != GCSADMM_OK) return rc;
    const int P = num_polytopes;
    DevBuf w, st;
    hipError_t e;
    CK(w.alloc(sizeof(double) * (size_t)P * (n + 1))); CK(st.alloc(sizeof(int) * (size_t)P));
    DISPATCH_N(n, (launch_ball<NN>(sc, P, nullptr, nullptr, nullptr, centre_rows(sc.maxm), 0.0, 0, w.as<double>(), nullptr, st.as<int>())));
    if (rc != GCSADMM_OK) return rc;
    std::vector<double> hw((size_t)P * (n + 1));
    std::vector<int> hs((size_t)P);
    CK(hipMemcpy(hw.data(), w.p, sizeof(double) * hw.size(), hipMemcpyDeviceToHost));
    CK(hipMemcpy(hs.data(), st.p, sizeof(int) * hs.size(), hipMemcpyDeviceToHost));
    for (int p = 0; p < P; ++p) {
        for (int k = 0; k < n; ++k) centers[(size_t)p * n + k] = hw[(size_t)p * (n + 1) + k];
        if (radii) radii[p] = hw[(size_t)p * (n + 1) + n];
        if (status) status[p] = hs[p];
    }
    return GCSADMM_OK;
}

int gcsadmm_polytope_bounds(int n, int num_polytopes, const int *poly_ptr, const double *poly_A, const double *poly_b,
                            const double *centers, int device, double *lo, double *hi, int *status)
{
    RestoreDevice restore_device_;
    if (!centers || !lo || !hi) { g_err = "null centres or output"; return GCSADMM_ERR_BAD_ARG; }
    Scene sc;
    int rc = upload_scene(sc, n, num_polytopes, poly_ptr, poly_A, poly_b, device);
    if (rc != GCSADMM_OK) return rc;
    const size_t P = (size_t)num_polytopes;
    DevBuf dc, dlo, dhi, st;
    hipError_t e;
    CK(dc.alloc(sizeof(double) * P * n)); CK(dlo.alloc(sizeof(double) * P * n)); CK(dhi.alloc(sizeof(double) * P * n));
    CK(st.alloc(sizeof(int) * P * 2 * n));
    CK(hipMemcpy(dc.p, centers, sizeof(double) * P * n, hipMemcpyHostToDevice));
    DISPATCH_N(n, (launch_bounds<NN>(sc, dc.as<double>(), dlo.as<double>(), dhi.as<double>(), st.as<int>())));
    if (rc != GCSADMM_OK) return rc;
    CK(hipMemcpy(lo, dlo.p, sizeof(double) * P * n, hipMemcpyDeviceToHost));
    CK(hipMemcpy(hi, dhi.p, sizeof(double) * P * n, hipMemcpyDeviceToHost));
    if (status) CK(hipMemcpy(status, st.p, sizeof(int) * P * 2 * n, hipMemcpyDeviceToHost));
    return GCSADMM_OK;
}

int gcsadmm_polytope_overlaps(int n, int num_polytopes, const int *poly_ptr, const double *poly_A, const double *poly_b,
                              const double *centers, long num_pairs, const int *pair_a, const int *pair_b, double tol,
                              int device, unsigned char *overlap, int *status)
{
    RestoreDevice restore_device_;
    if (num_pairs < 0 || (num_pairs > 0 && (!pair_a || !pair_b || !overlap))) { g_err = "null pair list or output"; return GCSADMM_ERR_BAD_ARG; }
    for (long t = 0; t < num_pairs; ++t)
        if (pair_a[t] < 0 || pair_a[t] >= num_polytopes || pair_b[t] < 0 || pair_b[t] >= num_polytopes) {
            g_err = "pair index out of range"; return GCSADMM_ERR_BAD_ARG;
        }
    Scene sc;
    int rc = upload_scene(sc, n, num_polytopes, poly_ptr, poly_A, poly_b, device);
    if (rc != GCSADMM_OK) return rc;
    const size_t P = (size_t)num_polytopes, T = (size_t)num_pairs;
    DevBuf da, db, dc, df, st;
    hipError_t e;
    CK(da.alloc(sizeof(int) * T)); CK(db.alloc(sizeof(int) * T)); CK(df.alloc(T)); CK(st.alloc(sizeof(int) * T));
    CK(hipMemcpy(da.p, pair_a, sizeof(int) * T, hipMemcpyHostToDevice));
    CK(hipMemcpy(db.p, pair_b, sizeof(int) * T, hipMemcpyHostToDevice));
    if (centers) {
        CK(dc.alloc(sizeof(double) * P * n));
        CK(hipMemcpy(dc.p, centers, sizeof(double) * P * n, hipMemcpyHostToDevice));
    }
    DISPATCH_N(n, (launch_ball<NN>(sc, num_pairs, da.as<int>(), db.as<int>(), centers ? dc.as<double>() : nullptr, overlap_rows(sc.maxm), tol, 1,
                                   nullptr, df.as<unsigned char>(), st.as<int>())));
    if (rc != GCSADMM_OK) return rc;
    CK(hipMemcpy(overlap, df.p, T, hipMemcpyDeviceToHost));
    if (status) CK(hipMemcpy(status, st.p, sizeof(int) * T, hipMemcpyDeviceToHost));
    return GCSADMM_OK;
}

int gcsadmm_scene_create(int n, int num_polytopes, const int *poly_ptr, const double *poly_A, const double *poly_b, int device,
                         gcsadmm_scene *out)
{
    RestoreDevice restore_device_;
    if (!out) { g_err = "null output"; return GCSADMM_ERR_BAD_ARG; }
    *out = nullptr;
    gcsadmm_scene_s *s = new (std::nothrow) gcsadmm_scene_s;
    if (!s) { g_err = "out of host memory"; return GCSADMM_ERR_NO_MEMORY; }
    int rc;
    try {
        rc = upload_scene(s->sc, n, num_polytopes, poly_ptr, poly_A, poly_b, device);
    } catch (const std::bad_alloc &) {
        g_err = "out of host memory"; rc = GCSADMM_ERR_NO_MEMORY;
    }
    if (rc == GCSADMM_OK) {
        s->n = n; s->P = num_polytopes; s->device = device;
        const size_t P = (size_t)num_polytopes, d = sizeof(double);
        hipError_t e = hipSuccess;
        const struct { DevBuf *buf; size_t bytes; } bufs[] = {
            {&s->w, d * P * (n + 1)}, {&s->cen, d * P * n}, {&s->rad, d * P}, {&s->st_c, sizeof(int) * P}, {&s->lo, d * P * n}, {&s->hi, d * P * n},
            {&s->st_b, sizeof(int) * P * 2 * n}, {&s->lo0, d * P}, {&s->order, sizeof(int) * P}, {&s->slo, d * P * n}, {&s->shi, d * P * n},
            {&s->count, sizeof(int) * P}, {&s->offset, sizeof(long long) * P}, {&s->counts, 2 * sizeof(unsigned long long)}};
        for (const auto &b : bufs)
            if (e == hipSuccess) e = b.buf->alloc(b.bytes);
        if (e != hipSuccess) { g_err = std::string("hipMalloc: ") + hipGetErrorString(e); rc = GCSADMM_ERR_HIP; }
    }
    if (rc != GCSADMM_OK) { delete s; return rc; }
    *out = s;
    return GCSADMM_OK;
}

void gcsadmm_scene_destroy(gcsadmm_scene s)
{
    RestoreDevice restore_device_;
    if (!s) return;
    (void)hipSetDevice(s->device);
    delete s;
}

int gcsadmm_scene_centers(gcsadmm_scene s, double *centers, double *radii, int *status)
{
    RestoreDevice restore_device_;
    int rc = enter_scene(s);
    if (rc != GCSADMM_OK) return rc;
    const int n = s->n, P = s->P;
    hipError_t e;
    s->have_centers = false;
    DISPATCH_N(n, (launch_ball<NN>(s->sc, P, nullptr, nullptr, nullptr, centre_rows(s->sc.maxm), 0.0, 0, s->w.as<double>(), nullptr, s->st_c.as<int>())));
    if (rc != GCSADMM_OK) return rc;
    if (P > 0) hipLaunchKernelGGL(split_centres_kernel, dim3(blocks_of(P)), dim3(TB), 0, 0, s->w.as<double>(), n, P, s->cen.as<double>(), s->rad.as<double>());
    CK(hipGetLastError());
    if (centers) CK(hipMemcpy(centers, s->cen.p, sizeof(double) * (size_t)P * n, hipMemcpyDeviceToHost));
    if (radii) CK(hipMemcpy(radii, s->rad.p, sizeof(double) * (size_t)P, hipMemcpyDeviceToHost));
    if (status) CK(hipMemcpy(status, s->st_c.p, sizeof(int) * (size_t)P, hipMemcpyDeviceToHost));
    CK(hipStreamSynchronize(nullptr));
    s->have_centers = true;
    return GCSADMM_OK;
}

int gcsadmm_scene_bounds(gcsadmm_scene s, double *lo, double *hi, int *status)
{
    RestoreDevice restore_device_;
    int rc = enter_scene(s);
    if (rc != GCSADMM_OK) return rc;
    if (!s->have_centers) { g_err = "no resident centres: call gcsadmm_scene_centers first"; return GCSADMM_ERR_BAD_ARG; }
    const int n = s->n, P = s->P;
    const size_t cells = (size_t)P * n;
    hipError_t e;
    s->have_boxes = s->have_pairs = s->have_overlaps = false;
    DISPATCH_N(n, (launch_bounds<NN>(s->sc, s->cen.as<double>(), s->lo.as<double>(), s->hi.as<double>(), s->st_b.as<int>())));
    if (rc != GCSADMM_OK) return rc;
    if (cells > 0)
        hipLaunchKernelGGL(open_failed_sides_kernel, dim3(blocks_of((long)cells * 2)), dim3(TB), 0, 0, s->st_b.as<int>(), n, P, s->lo.as<double>(),
                           s->hi.as<double>());
    CK(hipGetLastError());
    if (lo) CK(hipMemcpy(lo, s->lo.p, sizeof(double) * cells, hipMemcpyDeviceToHost));
    if (hi) CK(hipMemcpy(hi, s->hi.p, sizeof(double) * cells, hipMemcpyDeviceToHost));
    if (status) CK(hipMemcpy(status, s->st_b.p, sizeof(int) * cells * 2, hipMemcpyDeviceToHost));
    CK(hipStreamSynchronize(nullptr));
    s->have_boxes = true;
    return GCSADMM_OK;
}

int gcsadmm_scene_set_boxes(gcsadmm_scene s, const double *lo, const double *hi)
{
    RestoreDevice restore_device_;
    int rc = enter_scene(s);
    if (rc != GCSADMM_OK) return rc;
    const size_t cells = (size_t)s->P * s->n;
    if (cells > 0 && (!lo || !hi)) { g_err = "null boxes"; return GCSADMM_ERR_BAD_ARG; }
    for (size_t i = 0; i < cells; ++i)
        if (!(lo[i] <= hi[i])) { g_err = "box with a NaN or with lo > hi"; return GCSADMM_ERR_BAD_ARG; }
    hipError_t e;
    s->have_boxes = s->have_pairs = s->have_overlaps = false;
    CK(hipMemcpy(s->lo.p, lo, sizeof(double) * cells, hipMemcpyHostToDevice));
    CK(hipMemcpy(s->hi.p, hi, sizeof(double) * cells, hipMemcpyHostToDevice));
    s->have_boxes = true;
    return GCSADMM_OK;
}

static int candidate_pairs(gcsadmm_scene s, double pad, int64_t *num_pairs)
{
    int rc = enter_scene(s);
    if (rc != GCSADMM_OK) return rc;
    if (!s->have_boxes) { g_err = "no resident boxes: call gcsadmm_scene_bounds or gcsadmm_scene_set_boxes first"; return GCSADMM_ERR_BAD_ARG; }
    if (!(pad == pad)) { g_err = "pad is NaN"; return GCSADMM_ERR_BAD_ARG; }
    const int n = s->n, P = s->P;
    hipError_t e;
    s->have_pairs = s->have_overlaps = false;
    s->T = 0;
    // sort on the host (P log P on P doubles; a device radix sort would order -0.0 before +0.0 and change the order of ties)
    std::vector<double> lo0((size_t)P);
    std::vector<int> order((size_t)P), count((size_t)P);
    std::vector<long long> offset((size_t)P);
    if (P > 0) hipLaunchKernelGGL(first_lower_bounds_kernel, dim3(blocks_of(P)), dim3(TB), 0, 0, s->lo.as<double>(), n, P, s->lo0.as<double>());
    CK(hipGetLastError());
    CK(hipMemcpy(lo0.data(), s->lo0.p, sizeof(double) * (size_t)P, hipMemcpyDeviceToHost));
    for (int p = 0; p < P; ++p)      // a NaN has no place in the order (set_boxes refuses one; a bounds LP reports none with a status >= 0)
        if (!(lo0[p] == lo0[p])) { g_err = "resident box with a NaN lower bound"; return GCSADMM_ERR_BAD_ARG; }
    sweep_order(lo0.data(), P, order.data());
    CK(hipMemcpy(s->order.p, order.data(), sizeof(int) * (size_t)P, hipMemcpyHostToDevice));
    if (P > 0)
        hipLaunchKernelGGL(sweep_gather_kernel, dim3(blocks_of(P)), dim3(TB), 0, 0, s->lo.as<double>(), s->hi.as<double>(), s->order.as<int>(), n, P,
                           s->slo.as<double>(), s->shi.as<double>());
    CK(hipGetLastError());
    DISPATCH_N(n, (launch_sweep<NN>(s, false, pad)));
    if (rc != GCSADMM_OK) return rc;
    CK(hipMemcpy(count.data(), s->count.p, sizeof(int) * (size_t)P, hipMemcpyDeviceToHost));
    long long total = 0;
    if (!sweep_scan(count.data(), P, offset.data(), &total)) {      // before anything is allocated
        g_err = "more than 2^31 - 1 candidate pairs"; return GCSADMM_ERR_UNSUPPORTED;
    }
    CK(s->pa.alloc(sizeof(int) * (size_t)total)); CK(s->pb.alloc(sizeof(int) * (size_t)total));
    CK(s->flag.alloc((size_t)total)); CK(s->st_o.alloc(sizeof(int) * (size_t)total));
    CK(hipMemcpy(s->offset.p, offset.data(), sizeof(long long) * (size_t)P, hipMemcpyHostToDevice));
    if (total > 0) {
        DISPATCH_N(n, (launch_sweep<NN>(s, true, pad)));
        if (rc != GCSADMM_OK) return rc;
    }
    CK(hipStreamSynchronize(nullptr));
    s->T = total;
    s->have_pairs = true;
    if (num_pairs) *num_pairs = total;
    return GCSADMM_OK;
}

int gcsadmm_scene_candidate_pairs(gcsadmm_scene s, double pad, int64_t *num_pairs)
{
    RestoreDevice restore_device_;
    try {
        return candidate_pairs(s, pad, num_pairs);
    } catch (const std::bad_alloc &) {      // the host arrays of the sort and the scan
        g_err = "out of host memory"; return GCSADMM_ERR_NO_MEMORY;
    }
}

int gcsadmm_scene_overlaps(gcsadmm_scene s, double tol, int64_t *num_overlapping, int64_t *num_undecided)
{
    RestoreDevice restore_device_;
    int rc = enter_scene(s);
    if (rc != GCSADMM_OK) return rc;
    if (!s->have_pairs) { g_err = "no resident pairs: call gcsadmm_scene_candidate_pairs first"; return GCSADMM_ERR_BAD_ARG; }
    if (!s->have_centers) { g_err = "no resident centres: call gcsadmm_scene_centers first"; return GCSADMM_ERR_BAD_ARG; }
    const size_t T = (size_t)s->T;
    hipError_t e;
    s->have_overlaps = false;
    DISPATCH_N(s->n, (launch_ball<NN>(s->sc, (long)s->T, s->pa.as<int>(), s->pb.as<int>(), s->cen.as<double>(), overlap_rows(s->sc.maxm), tol, 1,
                                      nullptr, s->flag.as<unsigned char>(), s->st_o.as<int>())));
    if (rc != GCSADMM_OK) return rc;
    if (num_overlapping || num_undecided) {      // counted where the flags are: two numbers come back, the arrays stay for read_pairs
        unsigned long long counts[2] = {0, 0};
        CK(hipMemcpy(s->counts.p, counts, sizeof(counts), hipMemcpyHostToDevice));
        if (T > 0)
            hipLaunchKernelGGL(count_decisions_kernel, dim3(blocks_of((long)T)), dim3(TB), 0, 0, s->flag.as<unsigned char>(), s->st_o.as<int>(), (long)T,
                               s->counts.as<unsigned long long>());
        CK(hipGetLastError());
        CK(hipMemcpy(counts, s->counts.p, sizeof(counts), hipMemcpyDeviceToHost));
        if (num_overlapping) *num_overlapping = (int64_t)counts[0];
        if (num_undecided) *num_undecided = (int64_t)counts[1];
    }
    CK(hipStreamSynchronize(nullptr));
    s->have_overlaps = true;
    return GCSADMM_OK;
}

int gcsadmm_scene_read_pairs(gcsadmm_scene s, int *pair_a, int *pair_b, unsigned char *overlap, int *status)
{
    RestoreDevice restore_device_;
    int rc = enter_scene(s);
    if (rc != GCSADMM_OK) return rc;
    if (!s->have_pairs) { g_err = "no resident pairs: call gcsadmm_scene_candidate_pairs first"; return GCSADMM_ERR_BAD_ARG; }
    if ((overlap || status) && !s->have_overlaps) { g_err = "the resident pairs are not decided: call gcsadmm_scene_overlaps first"; return GCSADMM_ERR_BAD_ARG; }
    const size_t T = (size_t)s->T;
    hipError_t e;
    if (pair_a) CK(hipMemcpy(pair_a, s->pa.p, sizeof(int) * T, hipMemcpyDeviceToHost));
    if (pair_b) CK(hipMemcpy(pair_b, s->pb.p, sizeof(int) * T, hipMemcpyDeviceToHost));
    if (overlap) CK(hipMemcpy(overlap, s->flag.p, T, hipMemcpyDeviceToHost));
    if (status) CK(hipMemcpy(status, s->st_o.p, sizeof(int) * T, hipMemcpyDeviceToHost));
    return GCSADMM_OK;
}

} // extern "C"
