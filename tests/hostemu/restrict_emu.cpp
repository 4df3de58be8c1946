// restrict_emu.cpp -- the path-restriction solve of the HIP library (gcs_admm_amd/csrc/path_restrict_core.h) and its plan
// (restrict_plan.h) compiled for the host.  The executor runs the tasks of every barrier-separated phase one after the other, in
// ascending order or (reverse != 0) descending: equal results are evidence that the tasks of a phase are independent.  Unwritten
// workspace is poisoned with NaN.  Test-only (tests/test_path_restrict.py); the GPU tests are in tests/test_gpu_path_restrict.py.
#include <math.h>

#include <string>
#include <vector>

#include "restrict_plan.h"
#include "step_args.h"      // dispatch_dim

namespace {
struct HostExec {
    bool reverse;
    int tid() const { return 0; }
    int nthreads() const { return 1; }
    int task(int u, int count) const { return reverse ? count - 1 - u : u; }
    void sync() {}
    void reduce3(double &, double &, double &) {}
};
std::string g_err;
}  // namespace

extern "C" const char *restrict_emu_error(void) { return g_err.c_str(); }

// the plan alone: totals = (grid, threads, total_regions, total_points, total_rows, ws_doubles); row_prefix [regions + 2 paths] and
// ws_off [paths] may be null
extern "C" int restrict_emu_plan(int n, int P, const int *poly_ptr, int num_paths, const int *path_ptr, const int *path_poly, long long *totals,
                                 int *row_prefix, long long *ws_off)
{
    gcsadmm_k::RestrictPlan rp;
    const int rc = gcsadmm_k::make_restrict_plan(n, P, poly_ptr, num_paths, path_ptr, path_poly, rp, g_err);
    if (rc != GCSADMM_OK) return rc;
    totals[0] = rp.grid; totals[1] = rp.threads; totals[2] = rp.total_regions; totals[3] = rp.total_points; totals[4] = rp.total_rows;
    totals[5] = rp.ws_doubles;
    if (row_prefix) for (size_t i = 0; i < rp.row_prefix.size(); ++i) row_prefix[i] = rp.row_prefix[i];
    if (ws_off) for (size_t i = 0; i < rp.ws_off.size(); ++i) ws_off[i] = rp.ws_off[i];
    return rc;
}

extern "C" long long restrict_emu_ws_doubles(int n, long long k, long long R) { return gcs_restrict::restrict_ws_doubles(n, k, R); }

// gcsadmm_scene_restrict_paths on host arrays: same arguments after the scene's CSR, same return codes
extern "C" int restrict_emu_solve(int n, int P, const int *poly_ptr, const double *A, const double *b, int num_paths, const int *path_ptr,
                                  const int *path_poly, const double *start, double tol, int max_iter, int reverse, double *points, double *cost,
                                  int *iterations, int *status)
{
    gcsadmm_k::RestrictPlan rp;
    const int rc = gcsadmm_k::make_restrict_plan(n, P, poly_ptr, num_paths, path_ptr, path_poly, rp, g_err);
    if (rc != GCSADMM_OK) return rc;
    if (num_paths > 0 && (!start || !points || !cost || !iterations || !status)) { g_err = "null start or output"; return GCSADMM_ERR_BAD_ARG; }
    std::vector<double> ws((size_t)rp.ws_doubles, NAN);
    HostExec ex{reverse != 0};
    for (int p = 0; p < num_paths; ++p) {
        gcs_restrict::PathProblem pr;
        pr.k = path_ptr[p + 1] - path_ptr[p];
        pr.poly = path_poly + path_ptr[p];
        pr.rowp = rp.row_prefix.data() + path_ptr[p] + 2 * (size_t)p;
        pr.poly_ptr = poly_ptr; pr.A = A; pr.b = b;
        pr.start = start + (size_t)(path_ptr[p] + p) * n;
        pr.points = points + (size_t)(path_ptr[p] + p) * n;
        pr.tol = tol; pr.max_iter = max_iter;
        gcsadmm_k::dispatch_dim<1, 2, 3, 4, 5, 6, 7, 8>(n, [&](auto nn) {
            constexpr int N = decltype(nn)::value;
            std::vector<gcs_restrict::PathShared<N>> sh(1);
            status[p] = gcs_restrict::path_restrict_solve<N>(ex, pr, ws.data() + rp.ws_off[p], sh[0], cost + p, iterations + p);
        });
    }
    return GCSADMM_OK;
}
