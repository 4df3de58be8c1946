// HOST build of the split form of the workgroup program (gcs_admm_amd/csrc/vertex_wg.h wg_solve_vertex<..., SPLIT = true>: the units in
// a separate buffer, the stand-in for the handle's device-memory workspace) next to the in-LDS form, for tests/test_hostemu_split.py.
// Modelled on wg_emu.cpp: regions run their tasks serially, ascending or (-DGCS_WG_REVERSE) descending; unwritten LDS and unwritten
// units are poisoned with NaN.  Test-only; the product has no path into it.
#include <algorithm>
#include <vector>

#include "vertex_wg.h"

#ifdef GCS_WG_REVERSE
#define EMU_FN wg_split_emu_vertex_step_rev
#else
#define EMU_FN wg_split_emu_vertex_step
#endif

template <int N, bool BOX>
static void run_all(const gcs_wg::WgArgs<double> &a, bool split, int *status, int *iters)
{
    using W = std::conditional_t<BOX, gcs_wg::WLBox<N>, gcs_wg::WL<N>>;
    for (int w = 0; w < a.n_vtx; ++w) {
        const int v = a.vtx[w], d = a.inc_ptr[v + 1] - a.inc_ptr[v], m = a.poly_ptr[v + 1] - a.poly_ptr[v];
        std::vector<double> smem(split ? W::total(0, m) : W::total(d + 1, m), 0.0 / 0.0);
        std::vector<double> units(split ? W::units_doubles(d + 1, m) : 0, 0.0 / 0.0);
        int st = -9, it = 0;
        if (split) gcs_wg::wg_solve_vertex<N, double, BOX, true>(a, v, 1.0, 1.0, smem.data(), st, it, units.data());
        else gcs_wg::wg_solve_vertex<N, double, BOX, false>(a, v, 1.0, 1.0, smem.data(), st, it);
        status[v] = st; iters[v] = it;
        a.counters[0] += st != 0; a.counters[1] += it;
    }
}

// one vertex step (rho = mu_scale = 1) over the generic vertices; split: the split form; box: the BOX instantiation (n = 3, 6; the
// caller vouches for canonical boxes); warm / warm_ptr: warm-start records (warm_start.h) or null
extern "C" int EMU_FN(int split, int box, int n, int V, int E, int NI, const int *inc_ptr, const int *inc_edge, const int *inc_out,
                      const int *poly_ptr, const double *poly_A, const double *poly_b, const double *center, int src, int dst,
                      const double *zedge, const double *mu, double ipm_tol, int ipm_max_iter, double *warm, const long long *warm_ptr,
                      double *copy, double *xv, double *zv, double *yv, int *counters, int *status, int *iters)
{
    std::vector<int> deg_in(V, 0), vtx;
    for (int v = 0; v < V; ++v) {
        for (int k = inc_ptr[v]; k < inc_ptr[v + 1]; ++k) deg_in[v] += !inc_out[k];
        const int d = inc_ptr[v + 1] - inc_ptr[v];
        status[v] = 0; iters[v] = 0;
        if (!(v == src || v == dst || deg_in[v] == 0 || d - deg_in[v] == 0)) vtx.push_back(v);
    }
    std::vector<double> bc(poly_ptr[V]);
    for (int v = 0; v < V; ++v)
        for (int j = poly_ptr[v]; j < poly_ptr[v + 1]; ++j) {
            double s = poly_b[j];
            for (int k = 0; k < n; ++k) s -= poly_A[(size_t)j * n + k] * center[(size_t)v * n + k];
            bc[j] = s;
        }
    gcs_wg::WgArgs<double> a;
    a.n_vtx = (int)vtx.size(); a.vtx = vtx.data();
    gcsadmm_k::StepArgs<double> &s = a;
    s.inc_ptr = inc_ptr; s.deg_in = deg_in.data(); s.inc_edge = inc_edge; s.poly_ptr = poly_ptr;
    s.poly_A = poly_A; s.poly_bc = bc.data(); s.center = center; s.E = E; s.NI = NI;
    s.zedge = zedge; s.mu = mu; s.copy = copy; s.xv = xv; s.zv = zv; s.yv = yv; s.counters = counters;
    s.eps_edge = 1e-4; s.ipm_tol = ipm_tol; s.ipm_max_iter = ipm_max_iter; s.warm = warm; s.warm_ptr = warm_ptr;
    bool ran;
    if (box && gcs_wg::wg_has_box(n))
        ran = gcsadmm_k::dispatch_dim<3, 6>(n, [&](auto nn) { run_all<decltype(nn)::value, true>(a, split != 0, status, iters); });
    else
        ran = gcsadmm_k::dispatch_dim<1, 2, 3, 4, 5, 6, 7, 8>(n, [&](auto nn) { run_all<decltype(nn)::value, false>(a, split != 0, status, iters); });
    return ran ? 0 : 1;
}
