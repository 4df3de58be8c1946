// Host build of locate_box_kernel of csrc/scene_kernels.h (box_locate_core.h): the steps of gcsadmm_scene_locate_boxes with the 64 lanes
// of a workgroup run one after the other and the ballot formed from their 64 results.  Test infrastructure: never shipped, never timed.
#include <vector>
#include "box_locate_core.h"
using namespace gcsadmm_lp;

// locate_box_kernel<N, FILL> for workgroup (chunk, q)
template <int N, bool FILL>
static void locate_block(const LocateRegions &R, const double *boxes, long long chunks, long long limit, long long chunk, long long q, int *count,
                         const long long *offset, int *hit_region, unsigned char *hit_class)
{
    const double *c = boxes + (size_t)q * 2 * N, *hw = c + N;
    const size_t cell = (size_t)(q * chunks + chunk);
    long long pos = FILL ? offset[cell] : 0;
    int total = 0;
    for (int stride = 0; stride < LOCATE_CHUNK / LOCATE_WAVE; ++stride) {
        int region[LOCATE_WAVE], cls[LOCATE_WAVE];
        unsigned long long mask = 0;
        for (int lane = 0; lane < LOCATE_WAVE; ++lane) {
            region[lane] = locate_region(R.P, chunk, stride, lane);
            cls[lane] = locate_box_lane<N>(R, region[lane], c, hw);
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
static long long locate(int P, const int *ptr, const double *A, const double *b, int Q, const double *lo, const double *hi, double tol,
                        long long *hit_ptr, int *hit_region, unsigned char *hit_class, long long capacity)
{
    const LocateRegions R{P, ptr, A, b};
    std::vector<double> boxes((size_t)Q * 2 * N);
    for (long long q = 0; q < Q; ++q) locate_box_prepare(N, lo + (size_t)q * N, hi + (size_t)q * N, tol, boxes.data() + (size_t)q * 2 * N);
    const long long chunks = locate_chunks(P);
    const size_t cells = (size_t)(Q * chunks);
    std::vector<int> count(cells);
    std::vector<long long> offset(cells);
    std::vector<int64_t> hp((size_t)Q + 1, 0);
    for (long long q = 0; q < Q; ++q)
        for (long long c = 0; c < chunks; ++c) locate_block<N, false>(R, boxes.data(), chunks, 0, c, q, count.data(), nullptr, nullptr, nullptr);
    if (!locate_scan(count.data(), Q, chunks, offset.data(), hp.data())) return -1;
    const long long total = hp[(size_t)Q];
    if (hit_ptr)
        for (int q = 0; q <= Q; ++q) hit_ptr[q] = hp[(size_t)q];
    if (total > capacity) return total;
    for (long long q = 0; q < Q; ++q)
        for (long long c = 0; c < chunks; ++c)
            locate_block<N, true>(R, boxes.data(), chunks, total, c, q, nullptr, offset.data(), hit_region, hit_class);
    return total;
}

// the hit list of the boxes lo[Q][n], hi[Q][n] on the regions (ptr, A, b); returns the number of hits (-1: more than an int indexes),
// fills hit_ptr [Q + 1] and, when they have room for it (capacity entries each), hit_region / hit_class
extern "C" long long locate_box_emu_hits(int n, int P, const int *ptr, const double *A, const double *b, int Q, const double *lo, const double *hi,
                                         double tol, long long *hit_ptr, int *hit_region, unsigned char *hit_class, long long capacity)
{
    switch (n) {
    case 1: return locate<1>(P, ptr, A, b, Q, lo, hi, tol, hit_ptr, hit_region, hit_class, capacity);
    case 2: return locate<2>(P, ptr, A, b, Q, lo, hi, tol, hit_ptr, hit_region, hit_class, capacity);
    case 3: return locate<3>(P, ptr, A, b, Q, lo, hi, tol, hit_ptr, hit_region, hit_class, capacity);
    case 4: return locate<4>(P, ptr, A, b, Q, lo, hi, tol, hit_ptr, hit_region, hit_class, capacity);
    case 5: return locate<5>(P, ptr, A, b, Q, lo, hi, tol, hit_ptr, hit_region, hit_class, capacity);
    case 6: return locate<6>(P, ptr, A, b, Q, lo, hi, tol, hit_ptr, hit_region, hit_class, capacity);
    case 7: return locate<7>(P, ptr, A, b, Q, lo, hi, tol, hit_ptr, hit_region, hit_class, capacity);
    case 8: return locate<8>(P, ptr, A, b, Q, lo, hi, tol, hit_ptr, hit_region, hit_class, capacity);
    }
    return -99;
}

extern "C" int locate_box_emu_chunk(void) { return LOCATE_CHUNK; }

// the class of ONE (box, region) pair, straight from locate_box_classify: what a plain double loop over boxes and regions calls
template <int N> static int classify(const int *ptr, const double *A, const double *b, int region, const double *lo, const double *hi, double tol)
{
    double box[2 * N];
    locate_box_prepare(N, lo, hi, tol, box);
    return locate_box_classify<N>(LocateRegions{region + 1, ptr, A, b}, region, box, box + N);
}

extern "C" int locate_box_emu_class(int n, const int *ptr, const double *A, const double *b, int region, const double *lo, const double *hi, double tol)
{
    switch (n) {
    case 1: return classify<1>(ptr, A, b, region, lo, hi, tol);
    case 2: return classify<2>(ptr, A, b, region, lo, hi, tol);
    case 3: return classify<3>(ptr, A, b, region, lo, hi, tol);
    case 4: return classify<4>(ptr, A, b, region, lo, hi, tol);
    case 5: return classify<5>(ptr, A, b, region, lo, hi, tol);
    case 6: return classify<6>(ptr, A, b, region, lo, hi, tol);
    case 7: return classify<7>(ptr, A, b, region, lo, hi, tol);
    case 8: return classify<8>(ptr, A, b, region, lo, hi, tol);
    }
    return -99;
}
