// Host build of the device broad phase of csrc/polytope_lp.hip (box_sweep_core.h): the steps of gcsadmm_scene_candidate_pairs with
// the 64 lanes of a wavefront run one after the other and the ballot formed from their 64 results.  Test infrastructure: never
// shipped, never timed.
#include <vector>
#include "box_sweep_core.h"
using namespace gcsadmm_lp;

// sweep_kernel<N, FILL> for box k
template <int N, bool FILL>
static void sweep_box(const SortedBoxes &B, int k, double pad, int *count, const long long *offset, int *pair_a, int *pair_b)
{
    SweepBox<N> bk;
    sweep_load_box<N>(B, k, pad, bk);
    const int end = sweep_window_end(B.lo, B.P, bk.hip[0]);
    const int ok = FILL ? B.order[k] : 0;
    long long pos = FILL ? offset[k] : 0;
    int total = 0;
    for (int j0 = k + 1; j0 < end; j0 += SWEEP_WAVE) {
        bool hit[SWEEP_WAVE];
        unsigned long long mask = 0;
        for (int lane = 0; lane < SWEEP_WAVE; ++lane) {
            const int j = j0 + lane;
            hit[lane] = j < end && sweep_test<N>(B, bk, j, pad);
            if (hit[lane]) mask |= 1ull << lane;
        }
        if (FILL) {
            for (int lane = 0; lane < SWEEP_WAVE; ++lane)
                if (hit[lane]) sweep_store_pair(pair_a, pair_b, pos + sweep_rank(mask, lane), ok, B.order[j0 + lane]);
            pos += sweep_hits(mask);
        } else {
            total += sweep_hits(mask);
        }
    }
    if (!FILL) count[k] = total;
}

template <int N>
static long long sweep(int P, const double *lo, const double *hi, double pad, int *pair_a, int *pair_b, long long capacity)
{
    std::vector<double> lo0((size_t)P), slo((size_t)P * N), shi((size_t)P * N);
    std::vector<int> order((size_t)P), count((size_t)P);
    std::vector<long long> offset((size_t)P);
    for (int p = 0; p < P; ++p) lo0[p] = lo[(size_t)p * N];
    sweep_order(lo0.data(), P, order.data());
    for (int t = 0; t < P; ++t) sweep_gather(lo, hi, order.data(), N, P, t, slo.data(), shi.data());
    const SortedBoxes B{P, slo.data(), shi.data(), order.data()};
    for (int k = 0; k < P; ++k) sweep_box<N, false>(B, k, pad, count.data(), nullptr, nullptr, nullptr);
    long long total = 0;
    if (!sweep_scan(count.data(), P, offset.data(), &total)) return -1;
    if (total > capacity) return total;
    for (int k = 0; k < P; ++k) sweep_box<N, true>(B, k, pad, nullptr, offset.data(), pair_a, pair_b);
    return total;
}

// the pair list of boxes lo[P][n], hi[P][n]; returns the number of pairs (-1: too many for the narrow phase) and fills pair_a / pair_b
// when they have room for it (capacity entries each)
extern "C" long long sweep_emu_pairs(int n, int P, const double *lo, const double *hi, double pad, int *pair_a, int *pair_b, long long capacity)
{
    switch (n) {
    case 1: return sweep<1>(P, lo, hi, pad, pair_a, pair_b, capacity);
    case 2: return sweep<2>(P, lo, hi, pad, pair_a, pair_b, capacity);
    case 3: return sweep<3>(P, lo, hi, pad, pair_a, pair_b, capacity);
    case 4: return sweep<4>(P, lo, hi, pad, pair_a, pair_b, capacity);
    case 5: return sweep<5>(P, lo, hi, pad, pair_a, pair_b, capacity);
    case 6: return sweep<6>(P, lo, hi, pad, pair_a, pair_b, capacity);
    case 7: return sweep<7>(P, lo, hi, pad, pair_a, pair_b, capacity);
    case 8: return sweep<8>(P, lo, hi, pad, pair_a, pair_b, capacity);
    }
    return -99;
}

// sweep_scan as the library calls it: 1 if the narrow phase can take the total, 0 if not
extern "C" int sweep_emu_scan(const int *count, int P, long long *offset, long long *total)
{
    return sweep_scan(count, P, offset, total) ? 1 : 0;
}
