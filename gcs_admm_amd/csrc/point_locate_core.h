// point_locate_core.h -- which regions lie under a query point: the classification of one (point, region) pair and the pieces of the
// count and fill passes shared by locate_kernel (polytope_lp.hip) and its host build (tests/hostemu/locate_emu.cpp; the product path is
// the kernel).
//
// A terminal of a query is the box [p - eps, p + eps] (graph.convert_pt_to_polytope), connected to region r iff box and region share a
// point: one pair LP, decided on r* >= -tol.  For a point almost none of these LPs is needed.  For row i of the region, a_i x <= b_i:
//
//     g_i = a_i . p - b_i        s_i = sum_k |a_ik|        r_i = 2^-40 (sum_k |a_ik p_k| + |b_i|)
//
//   OUT        some row has g_i > (eps + 2 tol) s_i + r_i.  Every x within eps + tol of p (infinity norm) then has
//              a_i x - b_i >= g_i - (eps + tol) s_i > tol s_i >= tol |a_i|_2, so the pair LP's r* is below -tol;
//   IN         every row has g_i <= -r_i: p itself lies in the region;
//   UNDECIDED  otherwise -- a band about eps wide around each facet, and the point just beyond an acute vertex, where every row alone
//              admits a point of the box and all rows together do not.  These pairs alone go to the pair LP.
//
// r_i covers the rounding of g_i many times over ((n + 1) 2^-53 of the same sum).  g_i and r_i are one fma chain each, in index order,
// and the threshold is one fma: no product is left for the compiler to contract or not, so the host build and the kernel classify bit
// for bit alike.
//
// The list: one 64-lane workgroup per (chunk of LOCATE_CHUNK regions, point), one region per lane, the lanes striding the chunk by 64.
// The hits of a stride are compacted in lane order (ballot + prefix count) and the (point, chunk) segments are placed by an exclusive
// scan of their counts, points outermost: the list is ordered by point, then region index; no atomics, the same list on every run.
#pragma once
#include <math.h>
#include <stddef.h>
#include <stdint.h>
#if defined(__HIPCC__)
#define GCS_LOCATE_HD __host__ __device__ __forceinline__
#else
#define GCS_LOCATE_HD inline
#endif

// regions per workgroup: a multiple of the wavefront (profiles/queries/README.md has what it was measured against)
#ifndef GCS_LOCATE_CHUNK
#define GCS_LOCATE_CHUNK 256
#endif

namespace gcsadmm_lp {

constexpr int LOCATE_WAVE = 64;
constexpr int LOCATE_CHUNK = GCS_LOCATE_CHUNK;
static_assert(LOCATE_CHUNK > 0 && LOCATE_CHUNK % LOCATE_WAVE == 0, "a chunk is whole strides");
constexpr int LOCATE_OUT = 0, LOCATE_IN = 1, LOCATE_UNDECIDED = 2;

// the regions: the polytope CSR
struct LocateRegions {
    int P;
    const int *ptr;
    const double *A, *b;
};

inline long long locate_chunks(int P) { return ((long long)P + LOCATE_CHUNK - 1) / LOCATE_CHUNK; }

// margin = eps + 2 tol, formed once by the caller
template <int N> GCS_LOCATE_HD int locate_classify(const LocateRegions &R, int region, const double *p, double margin)
{
    const int first = R.ptr[region], last = R.ptr[region + 1];
    bool in = true;
    for (int i = first; i < last; ++i) {
        const double *a = R.A + (size_t)i * N;
        const double bi = R.b[i];
        double g = -bi, mag = fabs(bi), s = 0.0;
#pragma unroll
        for (int k = 0; k < N; ++k) {
            g = fma(a[k], p[k], g);
            mag = fma(fabs(a[k]), fabs(p[k]), mag);
            s += fabs(a[k]);
        }
        const double r = 0x1p-40 * mag;
        if (g > fma(margin, s, r)) return LOCATE_OUT;
        in = in && g <= -r;
    }
    return in ? LOCATE_IN : LOCATE_UNDECIDED;
}

// hits of one stride in the lanes below `lane`: the place of this lane's hit among the stride's
GCS_LOCATE_HD int locate_rank(unsigned long long mask, int lane)
{
#if defined(__HIP_DEVICE_COMPILE__)
    (void)lane;
    return (int)__builtin_amdgcn_mbcnt_hi((unsigned)(mask >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)mask, 0u));
#else
    return __builtin_popcountll(mask & ((1ull << lane) - 1ull));
#endif
}
GCS_LOCATE_HD int locate_hits(unsigned long long mask)
{
#if defined(__HIP_DEVICE_COMPILE__)
    return __popcll(mask);
#else
    return __builtin_popcountll(mask);
#endif
}

// One lane's part of one stride of workgroup (chunk, point).  The region of `lane` in stride `stride` of `chunk`, or -1 past the end:
GCS_LOCATE_HD int locate_region(int P, long long chunk, int stride, int lane)
{
    const long long j = chunk * LOCATE_CHUNK + (long long)stride * LOCATE_WAVE + lane;
    return j < P ? (int)j : -1;
}
// its class (OUT past the end) ...
template <int N> GCS_LOCATE_HD int locate_lane(const LocateRegions &R, int region, const double *p, double margin)
{
    return region >= 0 ? locate_classify<N>(R, region, p, margin) : LOCATE_OUT;
}
// ... and, in the fill pass, its store: pos is the workgroup's offset plus the hits of its earlier strides, mask the stride's ballot of
// "not OUT".  limit is the length of the list (the count pass ran the same tests, so no position reaches it)
GCS_LOCATE_HD void locate_store(int *hit_region, unsigned char *hit_class, long long pos, long long limit, unsigned long long mask, int lane,
                                int region, int cls)
{
    if (cls == LOCATE_OUT) return;
    const long long at = pos + locate_rank(mask, lane);
    if (at < limit) {
        hit_region[at] = region;
        hit_class[at] = (unsigned char)cls;
    }
}

// ---- host side ----
// exclusive scan of the (point, chunk) counts in 64 bits, points outermost: offset[cells], hit_ptr[num_points + 1].  false: more hits
// than the list can index with an int
inline bool locate_scan(const int *count, long long num_points, long long chunks, long long *offset, int64_t *hit_ptr)
{
    long long s = 0;
    for (long long q = 0; q < num_points; ++q) {
        hit_ptr[q] = s;
        for (long long c = 0; c < chunks; ++c) {
            offset[q * chunks + c] = s;
            s += count[q * chunks + c];
        }
    }
    hit_ptr[num_points] = s;
    return s <= (long long)INT32_MAX;
}

} // namespace gcsadmm_lp
