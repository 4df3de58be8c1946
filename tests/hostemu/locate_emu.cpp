// Host build of locate_kernel of csrc/polytope_lp.hip (point_locate_core.h): the steps of gcsadmm_scene_locate_points with the 64 lanes
// of a workgroup run one after the other and the ballot formed from their 64 results.  Test infrastructure: never shipped, never timed.
#include <vector>
#include "point_locate_core.h"
using namespace gcsadmm_lp;

// locate_kernel<N, FILL> for workgroup (chunk, q)
template <int N, bool FILL>
static void locate_block(const LocateRegions &R, const double *points, double margin, long long chunks, long long limit, long long chunk, long long q,
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
            cls[lane] = locate_lane<N>(R, region[lane], p, margin);
            if (cls[lane] != LOCATE_OUT) mask |= 1ull << lane;
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
static long long locate(int P, const int *ptr, const double *A, const double *b, int Q, const double *points, double eps, double tol,
                        long long *hit_ptr, int *hit_region, unsigned char *hit_class, long long capacity)
{
    const LocateRegions R{P, ptr, A, b};
    const double margin = eps + 2.0 * tol;
    const long long chunks = locate_chunks(P);
    const size_t cells = (size_t)(Q * chunks);
    std::vector<int> count(cells);
    std::vector<long long> offset(cells);
    std::vector<int64_t> hp((size_t)Q + 1, 0);
    for (long long q = 0; q < Q; ++q)
        for (long long c = 0; c < chunks; ++c) locate_block<N, false>(R, points, margin, chunks, 0, c, q, count.data(), nullptr, nullptr, nullptr);
    if (!locate_scan(count.data(), Q, chunks, offset.data(), hp.data())) return -1;
    const long long total = hp[(size_t)Q];
    if (hit_ptr)
        for (int q = 0; q <= Q; ++q) hit_ptr[q] = hp[(size_t)q];
    if (total > capacity) return total;
    for (long long q = 0; q < Q; ++q)
        for (long long c = 0; c < chunks; ++c)
            locate_block<N, true>(R, points, margin, chunks, total, c, q, nullptr, offset.data(), hit_region, hit_class);
    return total;
}

// the hit list of points[Q][n] on the regions (ptr, A, b); returns the number of hits (-1: more than an int indexes), fills hit_ptr
// [Q + 1] and, when they have room for it (capacity entries each), hit_region / hit_class
extern "C" long long locate_emu_hits(int n, int P, const int *ptr, const double *A, const double *b, int Q, const double *points, double eps,
                                     double tol, long long *hit_ptr, int *hit_region, unsigned char *hit_class, long long capacity)
{
    switch (n) {
    case 1: return locate<1>(P, ptr, A, b, Q, points, eps, tol, hit_ptr, hit_region, hit_class, capacity);
    case 2: return locate<2>(P, ptr, A, b, Q, points, eps, tol, hit_ptr, hit_region, hit_class, capacity);
    case 3: return locate<3>(P, ptr, A, b, Q, points, eps, tol, hit_ptr, hit_region, hit_class, capacity);
    case 4: return locate<4>(P, ptr, A, b, Q, points, eps, tol, hit_ptr, hit_region, hit_class, capacity);
    case 5: return locate<5>(P, ptr, A, b, Q, points, eps, tol, hit_ptr, hit_region, hit_class, capacity);
    case 6: return locate<6>(P, ptr, A, b, Q, points, eps, tol, hit_ptr, hit_region, hit_class, capacity);
    case 7: return locate<7>(P, ptr, A, b, Q, points, eps, tol, hit_ptr, hit_region, hit_class, capacity);
    case 8: return locate<8>(P, ptr, A, b, Q, points, eps, tol, hit_ptr, hit_region, hit_class, capacity);
    }
    return -99;
}

// locate_scan as the library calls it: 1 if the list can be indexed, 0 if not
extern "C" int locate_emu_scan(const int *count, long long num_points, long long chunks, long long *offset, long long *hit_ptr)
{
    std::vector<int64_t> hp((size_t)num_points + 1);
    const bool ok = locate_scan(count, num_points, chunks, offset, hp.data());
    for (long long q = 0; q <= num_points; ++q) hit_ptr[q] = hp[(size_t)q];
    return ok ? 1 : 0;
}

extern "C" int locate_emu_chunk(void) { return LOCATE_CHUNK; }
