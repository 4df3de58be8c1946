// Host build of project_list_kernel and project_solve_kernel of csrc/scene_kernels.h (point_project_core.h): the steps of
// gcsadmm_scene_project_points with the 64 lanes of a workgroup run one after the other and the ballot formed from their 64 results.
// Test infrastructure: never shipped, never timed.
#include <vector>
#include "point_project_core.h"
using namespace gcsadmm_lp;

// project_list_kernel<N, FILL> for workgroup (chunk, q)
template <int N, bool FILL>
static void list_block(const LocateRegions &R, const double *points, const double *radius, long long chunks, long long limit, long long chunk, long long q,
                       int *count, const long long *offset, int *hit_region, unsigned char *hit_class)
{
    const double *p = points + (size_t)q * N;
    const size_t cell = (size_t)(q * chunks + chunk);
    long long pos = FILL ? offset[cell] : 0;
    int total = 0;
    for (int stride = 0; stride < LOCATE_CHUNK / LOCATE_WAVE; ++stride) {
        int region[LOCATE_WAVE], cls[LOCATE_WAVE];
        unsigned long long mask = 0;
        for (int lane = 0; lane < LOCATE_WAVE; ++lane) {
            region[lane] = locate_region(R.P, chunk, stride, lane);
            cls[lane] = project_lane<N>(R, region[lane], p, radius[q]);
            if (cls[lane] != PROJECT_OUT) mask |= 1ull << lane;
        }
        if (FILL) {
            for (int lane = 0; lane < LOCATE_WAVE; ++lane) locate_store(hit_region, hit_class, pos, limit, mask, lane, region[lane], cls[lane]);
            pos += locate_hits(mask);
        } else {
            total += locate_hits(mask);
        }
    }
    if (!FILL) count[cell] = total;
}

template <int N>
static long long project(int P, const int *ptr, const double *A, const double *b, int Q, const double *points, const double *radius, int max_iter,
                         long long *hit_ptr, int *hit_region, unsigned char *hit_class, double *distance, double *nearest, int *status, int *iterations,
                         long long capacity)
{
    const LocateRegions R{P, ptr, A, b};
    std::vector<double> rad((size_t)Q, INFINITY);
    if (radius) rad.assign(radius, radius + Q);
    const long long chunks = locate_chunks(P);
    const size_t cells = (size_t)(Q * chunks);
    std::vector<int> count(cells);
    std::vector<long long> offset(cells);
    std::vector<int64_t> hp((size_t)Q + 1, 0);
    for (long long q = 0; q < Q; ++q)
        for (long long c = 0; c < chunks; ++c) list_block<N, false>(R, points, rad.data(), chunks, 0, c, q, count.data(), nullptr, nullptr, nullptr);
    if (!locate_scan(count.data(), Q, chunks, offset.data(), hp.data())) return -1;
    const long long total = hp[(size_t)Q];
    std::vector<long long> hpl(hp.begin(), hp.end());
    if (hit_ptr)
        for (int q = 0; q <= Q; ++q) hit_ptr[q] = hpl[(size_t)q];
    if (total > capacity) return total;
    for (long long q = 0; q < Q; ++q)
        for (long long c = 0; c < chunks; ++c)
            list_block<N, true>(R, points, rad.data(), chunks, total, c, q, nullptr, offset.data(), hit_region, hit_class);
    // project_solve_kernel<N>: workgroups of PROJECT_LANES entries in list order
    const ProjectOut out{distance, nearest, status, iterations};
    for (long long block = 0; block * PROJECT_LANES < total; ++block)
        for (int lane = 0; lane < PROJECT_LANES; ++lane) {
            const long long t = block * PROJECT_LANES + lane;
            if (t < total) project_entry<N>(R, points, rad.data(), hpl.data(), Q, hit_region, max_iter, t, out);
        }
    return total;
}

#define DIMS(call)                                                                                                                     \
    switch (n) {                                                                                                                       \
    case 1: return call(1); case 2: return call(2); case 3: return call(3); case 4: return call(4);                                    \
    case 5: return call(5); case 6: return call(6); case 7: return call(7); case 8: return call(8);                                    \
    }                                                                                                                                  \
    return -99;

// the whole call on the regions (ptr, A, b): returns the number of hits (-1: more than an int indexes), fills hit_ptr [Q + 1] and, when
// they have room for it (capacity entries each), the list and the four arrays of the solve.  radius null: +inf for every point
extern "C" long long project_emu_call(int n, int P, const int *ptr, const double *A, const double *b, int Q, const double *points, const double *radius,
                                      int max_iter, long long *hit_ptr, int *hit_region, unsigned char *hit_class, double *distance, double *nearest,
                                      int *status, int *iterations, long long capacity)
{
#define CALL(N) project<N>(P, ptr, A, b, Q, points, radius, max_iter, hit_ptr, hit_region, hit_class, distance, nearest, status, iterations, capacity)
    DIMS(CALL)
#undef CALL
}

extern "C" int project_emu_chunk(void) { return LOCATE_CHUNK; }

// ONE (point, region) pair, straight from project_classify and project_solve: what a plain double loop over points and regions calls.
// Returns the class; a candidate's x [n], d, status and iterations are filled
template <int N>
static int pair(const int *ptr, const double *A, const double *b, int region, const double *p, double radius, int max_iter, double *x, double *d, int *status,
                int *iterations)
{
    const LocateRegions R{region + 1, ptr, A, b};
    const int cls = project_classify<N>(R, region, p, radius);
    if (cls != PROJECT_OUT) *status = project_solve<N>(R, region, p, radius, max_iter, x, d, iterations);
    return cls;
}

extern "C" int project_emu_pair(int n, const int *ptr, const double *A, const double *b, int region, const double *p, double radius, int max_iter, double *x,
                                double *d, int *status, int *iterations)
{
#define CALL(N) pair<N>(ptr, A, b, region, p, radius, max_iter, x, d, status, iterations)
    DIMS(CALL)
#undef CALL
}
