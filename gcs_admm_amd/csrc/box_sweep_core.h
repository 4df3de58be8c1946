// box_sweep_core.h -- the broad phase of graph construction: sort-and-sweep over the first coordinate of the regions' boxes, the
// pieces shared by sweep_kernel (polytope_lp.hip) and its host build (tests/hostemu/sweep_emu.cpp; the product path is the kernel).
//
// Contract: the pair list equals scene.candidate_pairs(lo, hi, pad) element for element -- same pairs, same order, a < b.  That
// function enumerates the boxes in stable order of lo[:, 0]; box k of that order visits the window k+1 .. end_k of later boxes, where
// end_k = searchsorted(los, hi0_k + pad, side="right"), and keeps j when lo_k[d] <= hi_j[d] + pad and lo_j[d] <= hi_k[d] + pad for
// every d >= 1.  Coordinate 0 is tested through the window alone.  Here one 64-lane wavefront owns box k and strides its window by 64;
// the hits of a stride are compacted in lane order (ballot + prefix count), so the order inside a box is the host's, and the boxes'
// segments are placed by an exclusive scan of their counts: no atomics, the same list on every run.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <algorithm>
#if defined(__HIPCC__)
#define GCS_SWEEP_HD __host__ __device__ __forceinline__
#else
#define GCS_SWEEP_HD inline
#endif

namespace gcsadmm_lp {

constexpr int SWEEP_WAVE = 64;

// the boxes in sweep order, coordinate-major: lo[d * P + k], hi[d * P + k] of box order[k] (lanes read consecutive addresses)
struct SortedBoxes {
    int P;
    const double *lo, *hi;
    const int *order;      // [P] stable argsort of the first lower bounds
};

// box order[t] of the region-major boxes lo[P][n], hi[P][n] into slot t of the sorted arrays
GCS_SWEEP_HD void sweep_gather(const double *lo, const double *hi, const int *order, int n, int P, int t, double *slo, double *shi)
{
    const size_t o = (size_t)order[t] * n;
    for (int d = 0; d < n; ++d) {
        slo[(size_t)d * P + t] = lo[o + d];
        shi[(size_t)d * P + t] = hi[o + d];
    }
}

// numpy.searchsorted(los, key, side="right"): the first index whose value exceeds key (P if none does)
GCS_SWEEP_HD int sweep_window_end(const double *los, int P, double key)
{
    int a = 0, b = P;
    while (a < b) {
        const int mid = a + ((b - a) >> 1);
        if (los[mid] <= key) a = mid + 1;
        else b = mid;
    }
    return a;
}

// the sweeping box: its lower bounds and its padded upper bounds (hi + pad, rounded once, as the host forms it)
template <int N> struct SweepBox {
    double lo[N], hip[N];
};
template <int N> GCS_SWEEP_HD void sweep_load_box(const SortedBoxes &B, int k, double pad, SweepBox<N> &bk)
{
#pragma unroll
    for (int d = 0; d < N; ++d) {
        bk.lo[d] = B.lo[(size_t)d * B.P + k];
        bk.hip[d] = B.hi[(size_t)d * B.P + k] + pad;
    }
}

// do the padded boxes k and j meet in coordinates 1 .. N-1?
template <int N> GCS_SWEEP_HD bool sweep_test(const SortedBoxes &B, const SweepBox<N> &bk, int j, double pad)
{
    bool hit = true;
#pragma unroll
    for (int d = 1; d < N; ++d) {
        const double lo_j = B.lo[(size_t)d * B.P + j], hip_j = B.hi[(size_t)d * B.P + j] + pad;
        hit = hit && bk.lo[d] <= hip_j && lo_j <= bk.hip[d];
    }
    return hit;
}

// hits of one stride in the lanes below `lane`: the place of this lane's pair among the stride's
GCS_SWEEP_HD int sweep_rank(unsigned long long mask, int lane)
{
#if defined(__HIP_DEVICE_COMPILE__)
    (void)lane;
    return (int)__builtin_amdgcn_mbcnt_hi((unsigned)(mask >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)mask, 0u));
#else
    return __builtin_popcountll(mask & ((1ull << lane) - 1ull));
#endif
}
GCS_SWEEP_HD int sweep_hits(unsigned long long mask)
{
#if defined(__HIP_DEVICE_COMPILE__)
    return __popcll(mask);
#else
    return __builtin_popcountll(mask);
#endif
}

GCS_SWEEP_HD void sweep_store_pair(int *pair_a, int *pair_b, long long pos, int ok, int oj)
{
    pair_a[pos] = ok < oj ? ok : oj;
    pair_b[pos] = ok < oj ? oj : ok;
}

// ---- host side ----
// stable argsort of the first lower bounds, as numpy.argsort(kind="stable") orders them: -0.0 and +0.0 are a tie
inline void sweep_order(const double *lo0, int P, int *order)
{
    for (int k = 0; k < P; ++k) order[k] = k;
    std::stable_sort(order, order + P, [lo0](int a, int b) { return lo0[a] < lo0[b]; });
}

// exclusive scan of the boxes' counts in 64 bits.  false: more pairs than the narrow phase can take (its kernel counts in an int)
inline bool sweep_scan(const int *count, int P, long long *offset, long long *total)
{
    long long s = 0;
    for (int k = 0; k < P; ++k) {
        offset[k] = s;
        s += count[k];
    }
    *total = s;
    return s <= (long long)INT32_MAX;
}

} // namespace gcsadmm_lp
