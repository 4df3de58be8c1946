// restrict_plan.h -- what gcsadmm_scene_restrict_paths decides before it allocates anything: the argument checks, the per-path point,
// row and block offsets, the workspace sizes and the grid.  Host-only and HIP-free like create_plan.h and batch_plan.h, so that the
// offsets and sizes can be tested on a machine without a GPU (tests/hostemu/restrict_emu.cpp, tests/test_path_restrict.py).
//
// Path p visits the regions path_poly[path_ptr[p] .. path_ptr[p + 1]), k_p of them, and has k_p + 1 points and blocks and k_p segments:
//   points (start, points)  : offset (path_ptr[p] + p) * n doubles
//   row prefix (row_prefix) : k_p + 2 entries at path_ptr[p] + 2 p; entry j = rows before point j, the last = R_p.  Point j carries the
//                             rows of r_{j-1} (j >= 1), then those of r_j (j <= k_p - 1)
//   workspace               : ws_off[p] doubles into one slab of ws_doubles; restrict_ws_doubles(n, k_p, R_p) each, rounded up to
//                             32 doubles so that every path's arrays start on a 256-byte boundary
//   grid                    : one 64-lane workgroup per path
#pragma once
#include <limits.h>

#include <string>
#include <vector>

#include "gcsadmm.h"
#include "path_restrict_core.h"

namespace gcsadmm_k {

constexpr int RESTRICT_THREADS = 64;
constexpr long long RESTRICT_WS_ALIGN = 32;
constexpr long long RESTRICT_WS_MAX_DOUBLES = 1ll << 40;      // 8 TiB: beyond any device, and far from overflowing the sums below

struct RestrictPlan {
    int n = 0, num_paths = 0, grid = 0, threads = RESTRICT_THREADS;
    long long total_regions = 0, total_points = 0, total_rows = 0, ws_doubles = 0;
    std::vector<int> row_prefix;            // [total_regions + 2 num_paths]
    std::vector<long long> ws_off;          // [num_paths]
};

inline gcsadmm_status make_restrict_plan(int n, int num_polytopes, const int *poly_ptr, int num_paths, const int *path_ptr, const int *path_poly,
                                         RestrictPlan &rp, std::string &err)
{
    auto fail = [&](gcsadmm_status st, int p, const char *why) {
        err = p < 0 ? std::string(why) : "path " + std::to_string(p) + ": " + why;
        return st;
    };
    rp = RestrictPlan();
    if (n < 1 || n > 8) return fail(GCSADMM_ERR_UNSUPPORTED, -1, "path restrictions are instantiated for n = 1..8");
    if (num_paths < 0 || !path_ptr || !poly_ptr || num_polytopes < 0) return fail(GCSADMM_ERR_BAD_ARG, -1, "null or negative path arguments");
    if (path_ptr[0] != 0) return fail(GCSADMM_ERR_BAD_ARG, -1, "path_ptr[0] != 0");
    for (int p = 0; p < num_paths; ++p)
        if (path_ptr[p + 1] <= path_ptr[p]) return fail(GCSADMM_ERR_BAD_ARG, p, "a path needs at least one region");
    const long long regions = path_ptr[num_paths];
    if (regions > 0 && !path_poly) return fail(GCSADMM_ERR_BAD_ARG, -1, "null path_poly");
    for (long long i = 0; i < regions; ++i)
        if (path_poly[i] < 0 || path_poly[i] >= num_polytopes) return fail(GCSADMM_ERR_BAD_ARG, -1, "region index out of range");
    // the totals, in 64 bits, before anything is sized by them
    long long rows = 0, ws = 0;
    for (int p = 0; p < num_paths; ++p) {
        const int k = path_ptr[p + 1] - path_ptr[p];
        long long R = 0;
        for (int j = 0; j < k; ++j) { const int r = path_poly[path_ptr[p] + j]; R += 2ll * (poly_ptr[r + 1] - poly_ptr[r]); }
        if (R > INT_MAX) return fail(GCSADMM_ERR_UNSUPPORTED, p, "more than 2^31 - 1 rows on one path");
        rows += R;
        long long w = gcs_restrict::restrict_ws_doubles(n, k, R);
        w = (w + RESTRICT_WS_ALIGN - 1) / RESTRICT_WS_ALIGN * RESTRICT_WS_ALIGN;
        ws += w;
        if (ws > RESTRICT_WS_MAX_DOUBLES) return fail(GCSADMM_ERR_UNSUPPORTED, p, "the workspace of the paths exceeds 2^40 doubles");
    }
    const long long points = regions + num_paths;
    if (points * n > INT_MAX || regions + 2ll * num_paths > INT_MAX) return fail(GCSADMM_ERR_UNSUPPORTED, -1, "more than 2^31 - 1 point coordinates in one call");
    rp.n = n; rp.num_paths = num_paths; rp.grid = num_paths;
    rp.total_regions = regions; rp.total_points = points; rp.total_rows = rows;
    rp.row_prefix.resize((size_t)(regions + 2ll * num_paths));
    rp.ws_off.resize((size_t)num_paths);
    ws = 0;
    for (int p = 0; p < num_paths; ++p) {
        const int k = path_ptr[p + 1] - path_ptr[p];
        const int *poly = path_poly + path_ptr[p];
        int *pre = rp.row_prefix.data() + path_ptr[p] + 2 * (size_t)p;
        int R = 0;
        for (int j = 0; j <= k; ++j) {
            pre[j] = R;
            if (j >= 1) R += poly_ptr[poly[j - 1] + 1] - poly_ptr[poly[j - 1]];
            if (j < k) R += poly_ptr[poly[j] + 1] - poly_ptr[poly[j]];
        }
        pre[k + 1] = R;
        rp.ws_off[p] = ws;
        const long long w = gcs_restrict::restrict_ws_doubles(n, k, R);
        ws += (w + RESTRICT_WS_ALIGN - 1) / RESTRICT_WS_ALIGN * RESTRICT_WS_ALIGN;
    }
    rp.ws_doubles = ws;
    return GCSADMM_OK;
}

}  // namespace gcsadmm_k
