// Host build of the set kernels of csrc/scene_kernels.h (informed_set_core.h): the steps of gcsadmm_scene_region_paths_sets and
// gcsadmm_scene_informed_regions_sets on arrays handed in, with the same checks and the same round loop -- the 256 lanes of a round run
// one after the other, forwards or backwards, each over the vertices it owns under the bound it read ahead of the round; the goal
// costs are folded into the bound behind every round.  Test infrastructure: never shipped, never timed.
#include <algorithm>
#include <string>
#include <vector>
#include "informed_set_core.h"
using namespace gcsadmm_lp;

static thread_local std::string g_err;

extern "C" {

const char *inf_set_emu_last_error(void) { return g_err.c_str(); }
double inf_set_emu_dist(int n, const double *c, const double *tlo, const double *thi) { return set_point_distance(c, tlo, thi, n); }
double inf_set_emu_gap(int n, const double *tlo, const double *thi, const double *lo, const double *hi, double pad) { return set_box_gap(tlo, thi, lo, hi, n, pad); }

// terminal_set_path_kernel, one workgroup after the other.  order: bit 0 the lanes backwards, bit 1 every round reads the bound of the
// round before (the lag a lane of the kernel may see).  d_out[B][P] (or null): the distances the search left; rounds[B] (or null):
// rounds run, the last one, which stored nothing, included
int inf_set_emu_paths(int P, int n, const long long *row_ptr, const int *head, const double *w, const double *centers, int B, const double *lo,
                      const double *hi, const long long *term_ptr, const int *term_region, int max_len, int order, int *path_region, int *path_len,
                      double *path_cost, int *status, double *d_out, int *rounds)
{
    if (const int rc = set_check_paths(P, n, B, lo, hi, term_ptr, term_region, max_len, g_err)) return rc;
    if (B == 0) return QUERY_OK;
    if (!path_region || !path_len || !path_cost || !status) { g_err = "null output array"; return QUERY_BAD_ARG; }
    const PathGraph g{P, n, row_ptr, head, w, centers};
    std::vector<double> d((size_t)std::max(P, 1));
    std::fill(path_region, path_region + (size_t)B * max_len, -1);
    for (int i = 0; i < B; ++i) {
        const SetQuery q = set_query(lo, hi, term_ptr, term_region, B, n, i);
        double bound = INFINITY, before = INFINITY;
        auto fold = [&] {
            before = bound;
            for (int j = 0; j < q.b; ++j) {
                const double c = set_goal_cost(g, q, d.data(), q.rt[j]);
                if (set_lowers(c, bound)) bound = c;
            }
        };
        for (int v = 0; v < P; ++v) d[v] = set_init(g, q, v);
        fold();
        int round = 0;
        for (; round < P; ++round) {
            const double U = (order & 2) ? before : bound;
            bool changed = false;
            for (int k = 0; k < PATH_THREADS; ++k) {
                const int t = (order & 1) ? PATH_THREADS - 1 - k : k;
                for (int v = t; v < P; v += PATH_THREADS) changed |= set_relax(g, d.data(), v, U);
            }
            if (!changed) { ++round; break; }
            fold();
        }
        if (rounds) rounds[i] = round;
        if (d_out) std::copy(d.begin(), d.begin() + P, d_out + (size_t)i * P);
        status[i] = set_backtrack(g, q, d.data(), max_len, path_region + (size_t)i * max_len, path_len + i, path_cost + i);
    }
    return QUERY_OK;
}

// terminal_set_keep_kernel and the count on the host
int inf_set_emu_keep(int P, int n, const double *lo, const double *hi, int B, const double *tlo, const double *thi, const double *bound, double pad,
                     unsigned char *keep, long long *num_kept)
{
    if (const int rc = set_check_keep(n, B, tlo, thi, bound, pad, g_err)) return rc;
    if (B == 0) return QUERY_OK;
    if (!keep) { g_err = "null output array"; return QUERY_BAD_ARG; }
    for (int i = 0; i < B; ++i) {
        const SetQuery q = set_query(tlo, thi, nullptr, nullptr, B, n, i);
        long long kept = 0;
        for (int r = 0; r < P; ++r)
            kept += keep[(size_t)i * P + r] = informed_keep(set_lower_bound(q, lo + (size_t)r * n, hi + (size_t)r * n, n, pad), bound[i]) ? 1 : 0;
        if (num_kept) num_kept[i] = kept;
    }
    return QUERY_OK;
}

} // extern "C"
