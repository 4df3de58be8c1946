// Host build of the informed-set kernels of csrc/scene_kernels.h (informed_core.h): the steps of gcsadmm_scene_region_paths and
// gcsadmm_scene_informed_regions on arrays handed in, with the same checks and the same round loop -- the 256 lanes of a round run one
// after the other, forwards (order 0) or backwards (order 1), each over the vertices it owns.  Test infrastructure: never shipped,
// never timed.
#include <algorithm>
#include <string>
#include <vector>
#include "informed_core.h"
using namespace gcsadmm_lp;

static thread_local std::string g_err;

extern "C" {

const char *inf_emu_last_error(void) { return g_err.c_str(); }
int inf_emu_chunk(int P) { return informed_chunk(P); }

// region_weight_kernel
void inf_emu_weights(int n, const double *centers, long long E, const int *tail, const int *head, double *w)
{
    for (long long p = 0; p < E; ++p) w[p] = informed_weight(centers, n, tail, head, p);
}

// region_path_kernel, one workgroup after the other.  d_out[B][P] (or null): the settled distances; rounds[B] (or null): rounds run,
// the last one, which changed nothing, included
int inf_emu_paths(int P, int n, const long long *row_ptr, const int *head, const double *w, const double *centers, int B, const double *points,
                  const long long *term_ptr, const int *term_region, int max_len, int order, int *path_region, int *path_len, double *path_cost,
                  int *status, double *d_out, int *rounds)
{
    if (const int rc = informed_check_paths(P, n, B, points, term_ptr, term_region, max_len, g_err)) return rc;
    if (B == 0) return QUERY_OK;
    if (!path_region || !path_len || !path_cost || !status) { g_err = "null output array"; return QUERY_BAD_ARG; }
    const PathGraph g{P, n, row_ptr, head, w, centers};
    std::vector<double> d((size_t)std::max(P, 1));
    std::fill(path_region, path_region + (size_t)B * max_len, -1);
    for (int i = 0; i < B; ++i) {
        PathQuery q;
        q.s = points + (size_t)i * n; q.g = points + (size_t)(B + i) * n;
        q.rs = term_region + term_ptr[i]; q.a = (int)(term_ptr[i + 1] - term_ptr[i]);
        q.rt = term_region + term_ptr[B + i]; q.b = (int)(term_ptr[B + i + 1] - term_ptr[B + i]);
        for (int v = 0; v < P; ++v) d[v] = informed_init(g, q, v);
        int round = 0;
        for (; round < P; ++round) {
            bool changed = false;
            for (int k = 0; k < PATH_THREADS; ++k) {
                const int t = order ? PATH_THREADS - 1 - k : k;
                for (int v = t; v < P; v += PATH_THREADS) changed |= informed_relax(g, d.data(), v);
            }
            if (!changed) { ++round; break; }
        }
        if (rounds) rounds[i] = round;
        if (d_out) std::copy(d.begin(), d.begin() + P, d_out + (size_t)i * P);
        status[i] = informed_backtrack(g, q, d.data(), max_len, path_region + (size_t)i * max_len, path_len + i, path_cost + i);
    }
    return QUERY_OK;
}

// informed_keep_kernel and the count on the host
int inf_emu_keep(int P, int n, const double *lo, const double *hi, int B, const double *points, const double *bound, double pad, unsigned char *keep,
                 long long *num_kept)
{
    if (const int rc = informed_check_keep(n, B, points, bound, pad, g_err)) return rc;
    if (B == 0) return QUERY_OK;
    if (!keep) { g_err = "null output array"; return QUERY_BAD_ARG; }
    for (int i = 0; i < B; ++i) {
        long long kept = 0;
        for (int r = 0; r < P; ++r) {
            const double lb = informed_lower_bound(points + (size_t)i * n, points + (size_t)(B + i) * n, lo + (size_t)r * n, hi + (size_t)r * n, n, pad);
            kept += keep[(size_t)i * P + r] = informed_keep(lb, bound[i]) ? 1 : 0;
        }
        if (num_kept) num_kept[i] = kept;
    }
    return QUERY_OK;
}

} // extern "C"
