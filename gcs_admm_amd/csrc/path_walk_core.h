// path_walk_core.h -- the candidate paths of the rounding step drawn on the device: the rule of one walk and the pieces shared by
// walk_kernel (path_walk.hip) and its host build (tests/hostemu/walk_emu.cpp; the product path is the kernel).  The pure Python
// restatement gcs_admm_amd/walks.py::walk_reference is the specification both are held to.
//
// A problem is a directed graph with src, dst and out-lists in edge order (a stable sort of the edges by tail): out-list entry k of
// vertex v, out_ptr[v] <= k < out_ptr[v + 1], has the head vertex out_head[k] and reads the activation y[out_edge[k]] (f64 or f32, a
// row of the solver's edge words, where the solver left it).
//
// Weight of an entry -- an exact integer, so that any summation order gives the same total and the kernel may reduce in parallel:
//     y is widened to double;  w = 0 if !(y > 0) (NaN, negatives, zero);  otherwise w = (uint64) floor(min(y, 2) * 2^40);
//     an entry whose head is already on the path has w = 0.
// Activations below 2^-40 therefore count as absent (the host walk of rounding.py draws the line at 1e-15: on purpose, documented
// in DESIGN.md).  An out-degree above 2^22 is refused, so a total stays at or below 2^63.
//
// Step at vertex v != dst, position j of the path (src is position 0), tot = sum of w over v's out-list:
//     tot == 0                  dead end: status 1, the path so far is kept;
//     the path has max_len      status 2, the first max_len vertices are kept;
//     walk 0                    the most probable path: the entry of largest w, among equal w the LAST in out-list order (the host's
//                               max((y, k)));
//     walk w >= 1               z = mix(seed, w, j), r = mulhi64(z, tot); the FIRST entry in out-list order whose inclusive prefix sum
//                               exceeds r.
// mix is splitmix64 on the counter (w << 32) + j + 1:
//     z = seed + 0x9E3779B97F4A7C15 * ((w << 32) + j + 1)   (mod 2^64)
//     z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9;  z = (z ^ (z >> 27)) * 0x94D049BB133111EB;  z = z ^ (z >> 31)
// so every (problem, walk) pair is independent of every other: no generator state passes from one walk to the next.
// Reaching dst gives status 0; src == dst gives the path [src] with status 0.
//
// One 64-lane workgroup runs one walk.  The lanes stride the out-list by 64: a first pass forms tot (and walk 0's maximum), a second
// one scans stride by stride and stops at the stride that holds the pick (ballot of "prefix sum > r", first set lane).  The visited set
// is a bitmap in LDS.  After the one exact scaling by 2^40 everything is integer arithmetic: there is nothing for the compiler to
// contract, and host build and kernel agree element for element.
#pragma once
#include <stddef.h>
#include <stdint.h>
#if defined(__HIPCC__)
#define GCS_WALK_HD __host__ __device__ __forceinline__
#else
#define GCS_WALK_HD inline
#endif

namespace gcsadmm_walk {

constexpr int WALK_WAVE = 64;
constexpr int WALK_MAX_VERTICES = 524288;      // the bitmap of one problem: 64 KB of LDS
constexpr int WALK_MAX_DEGREE = 1 << 22;       // 2^22 weights of at most 2^41
constexpr int WALK_OK = 0, WALK_DEAD_END = 1, WALK_TOO_LONG = 2;

inline size_t walk_bitmap_words(long long vertices) { return (size_t)((vertices + 31) / 32); }

GCS_WALK_HD uint64_t walk_weight(double y)
{
    if (!(y > 0.0)) return 0;
    return (uint64_t)((y < 2.0 ? y : 2.0) * 0x1p40);
}

GCS_WALK_HD uint64_t walk_mix(uint64_t seed, uint32_t walk, uint32_t j)
{
    uint64_t z = seed + 0x9E3779B97F4A7C15ull * (((uint64_t)walk << 32) + j + 1ull);
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}

GCS_WALK_HD uint64_t walk_mulhi(uint64_t a, uint64_t b)
{
#if defined(__HIP_DEVICE_COMPILE__)
    return __umul64hi(a, b);
#else
    return (uint64_t)(((unsigned __int128)a * b) >> 64);
#endif
}

GCS_WALK_HD bool walk_visited(const uint32_t *bitmap, int v) { return (bitmap[v >> 5] >> (v & 31)) & 1u; }
GCS_WALK_HD void walk_visit(uint32_t *bitmap, int v) { bitmap[v >> 5] |= 1u << (v & 31); }      // one lane marks, between two barriers

// One lane's part of a stride: out-list entry k of the current vertex (end: one past its last entry), its head and its weight
struct WalkItem {
    uint64_t w;
    int head;
};
template <class T> GCS_WALK_HD WalkItem walk_item(const int *out_head, const int *out_edge, const T *y, const uint32_t *bitmap, int k, int end)
{
    if (k >= end) return WalkItem{0, -1};
    const int head = out_head[k];
    return WalkItem{walk_visited(bitmap, head) ? 0 : walk_weight((double)y[out_edge[k]]), head};
}

// walk 0's order on (weight, out-list index): lexicographic
GCS_WALK_HD bool walk_better(uint64_t w, int k, uint64_t than_w, int than_k) { return w > than_w || (w == than_w && k > than_k); }

// the first set lane of a stride's ballot (the caller has found it non-zero)
GCS_WALK_HD int walk_first_lane(unsigned long long mask)
{
#if defined(__HIP_DEVICE_COMPILE__)
    return __ffsll((long long)mask) - 1;
#else
    return __builtin_ctzll(mask);
#endif
}

// ---- the 64 lanes together: wave intrinsics on the device, a loop over the lanes' values in the host build (a plain C++ compiler) ----
#if defined(__HIPCC__)
// exact total of the lanes' values, in every lane
__device__ __forceinline__ uint64_t walk_wave_sum(uint64_t x)
{
    for (int off = WALK_WAVE / 2; off > 0; off >>= 1) x += __shfl_xor((unsigned long long)x, off, WALK_WAVE);
    return x;
}
// inclusive prefix sum over the lanes
__device__ __forceinline__ uint64_t walk_wave_scan(uint64_t x, int lane)
{
    for (int off = 1; off < WALK_WAVE; off <<= 1) {
        const uint64_t below = __shfl_up((unsigned long long)x, off, WALK_WAVE);
        if (lane >= off) x += below;
    }
    return x;
}
// the lane whose inclusive prefix sum first exceeds r, -1 if none does
__device__ __forceinline__ int walk_wave_pick(uint64_t inclusive, uint64_t r)
{
    const unsigned long long mask = __ballot(inclusive > r);
    return mask ? walk_first_lane(mask) : -1;
}
// the largest (w, k) of the lanes, in every lane
__device__ __forceinline__ void walk_wave_max(uint64_t &w, int &k)
{
    for (int off = WALK_WAVE / 2; off > 0; off >>= 1) {
        const uint64_t ow = __shfl_xor((unsigned long long)w, off, WALK_WAVE);
        const int ok = __shfl_xor(k, off, WALK_WAVE);
        if (walk_better(ow, ok, w, k)) { w = ow; k = ok; }
    }
}
#else
inline uint64_t walk_wave_sum(const uint64_t *x)
{
    uint64_t s = 0;
    for (int lane = 0; lane < WALK_WAVE; ++lane) s += x[lane];
    return s;
}
inline void walk_wave_scan(const uint64_t *x, uint64_t *inclusive)
{
    uint64_t s = 0;
    for (int lane = 0; lane < WALK_WAVE; ++lane) inclusive[lane] = s += x[lane];
}
inline int walk_wave_pick(const uint64_t *inclusive, uint64_t r)
{
    unsigned long long mask = 0;
    for (int lane = 0; lane < WALK_WAVE; ++lane)
        if (inclusive[lane] > r) mask |= 1ull << lane;
    return mask ? walk_first_lane(mask) : -1;
}
inline void walk_wave_max(const uint64_t *w, const int *k, uint64_t &best_w, int &best_k)
{
    best_w = w[0]; best_k = k[0];
    for (int lane = 1; lane < WALK_WAVE; ++lane)
        if (walk_better(w[lane], k[lane], best_w, best_k)) { best_w = w[lane]; best_k = k[lane]; }
}
#endif

// ---- host side: the checks of gcsadmm_walks_create on one problem (V vertices, E edges, local ids).  0, or the status with `why` set ----
inline int walk_check_problem(long long V, long long E, const int *out_ptr, const int *out_head, const int *out_edge, int src, int dst,
                              const char *&why, long long &at)
{
    at = -1;
    if (V > WALK_MAX_VERTICES) { why = "more than 524288 vertices (the visited bitmap is 64 KB of LDS)"; return 2; }
    if (V < 1 || E < 0 || E > INT32_MAX) { why = "a problem needs at least one vertex and at most 2^31 - 1 edges"; return 1; }
    if (out_ptr[0] != 0 || out_ptr[V] != E) { why = "out_ptr does not run from 0 to the number of edges"; return 1; }
    for (long long v = 0; v < V; ++v) {
        if (out_ptr[v + 1] < out_ptr[v]) { why = "out_ptr is not monotone at vertex"; at = v; return 1; }
        if (out_ptr[v + 1] - out_ptr[v] > WALK_MAX_DEGREE) { why = "out-degree above 2^22 at vertex"; at = v; return 2; }
    }
    for (long long k = 0; k < E; ++k) {
        if (out_head[k] < 0 || out_head[k] >= V) { why = "head out of range at out-list entry"; at = k; return 1; }
        if (out_edge[k] < 0 || out_edge[k] >= E) { why = "edge id out of range at out-list entry"; at = k; return 1; }
    }
    if (src < 0 || src >= V || dst < 0 || dst >= V) { why = "src or dst out of range"; return 1; }
    return 0;
}

} // namespace gcsadmm_walk
