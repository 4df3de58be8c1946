// Host build of segment_clip_kernel and segment_chain_kernel of csrc/scene_kernels.h (segment_clip_core.h): the steps of
// gcsadmm_scene_clip_segments with the 64 lanes of a workgroup run one after the other, the ballot formed from their 64 results and the
// butterfly of the wave reduction run on an array of 64 lanes.  Test infrastructure: never shipped, never timed.
#include <algorithm>
#include <vector>
#include "segment_clip_core.h"
using namespace gcsadmm_lp;

// segment_clip_kernel<N, FILL> for workgroup (chunk, q)
template <int N, bool FILL>
static void clip_block(const LocateRegions &R, const double *from, const double *to, double tol, long long chunks, long long limit, long long chunk, long long q,
                       int *count, const long long *offset, int *hit_region, unsigned char *hit_class, double *hit_in, double *hit_out)
{
    const double *p = from + (size_t)q * N;
    double d[N];
    clip_direction<N>(p, to + (size_t)q * N, d);
    const size_t cell = (size_t)(q * chunks + chunk);
    long long pos = FILL ? offset[cell] : 0;
    int total = 0;
    for (int stride = 0; stride < LOCATE_CHUNK / LOCATE_WAVE; ++stride) {
        int region[LOCATE_WAVE], cls[LOCATE_WAVE];
        double t_in[LOCATE_WAVE] = {}, t_out[LOCATE_WAVE] = {};
        unsigned long long mask = 0;
        for (int lane = 0; lane < LOCATE_WAVE; ++lane) {
            region[lane] = locate_region(R.P, chunk, stride, lane);
            cls[lane] = clip_lane<N>(R, region[lane], p, d, tol, &t_in[lane], &t_out[lane]);
            if (cls[lane] != CLIP_OUT) mask |= 1ull << lane;
        }
        if (FILL) {
            for (int lane = 0; lane < LOCATE_WAVE; ++lane)
                clip_store(hit_region, hit_class, hit_in, hit_out, pos, limit, mask, lane, region[lane], cls[lane], t_in[lane], t_out[lane]);
            pos += locate_hits(mask);
        } else {
            total += locate_hits(mask);
        }
    }
    if (!FILL) count[cell] = total;
}

// segment_chain_kernel for the wavefront of segment q
static void chain_block(const long long *hit_ptr, const double *hit_in, const double *hit_out, long long q, int *status, double *reach, int *chain_len,
                        int *chain_hit)
{
    const long long first = hit_ptr[q];
    const int count = (int)(hit_ptr[q + 1] - first);
    const double *t_in = hit_in + first, *t_out = hit_out + first;
    double first_in[LOCATE_WAVE], first_out[LOCATE_WAVE];
    for (int lane = 0; lane < LOCATE_WAVE; ++lane) {
        first_in[lane] = lane < count ? t_in[lane] : 0.0;
        first_out[lane] = lane < count ? t_out[lane] : 0.0;
    }
    double cur = 0.0;
    int len = 0, st = COVER_COVERED;
    while (cur < 1.0) {
        double best_out[LOCATE_WAVE];
        int best_pos[LOCATE_WAVE];
        for (int lane = 0; lane < LOCATE_WAVE; ++lane)
            chain_lane_best(t_in, t_out, count, lane, first_in[lane], first_out[lane], cur, &best_out[lane], &best_pos[lane]);
        for (int off = LOCATE_WAVE / 2; off > 0; off >>= 1) {      // __shfl_xor: every lane reads its partner's value of before the step
            double other_out[LOCATE_WAVE];
            int other_pos[LOCATE_WAVE];
            for (int lane = 0; lane < LOCATE_WAVE; ++lane) { other_out[lane] = best_out[lane ^ off]; other_pos[lane] = best_pos[lane ^ off]; }
            for (int lane = 0; lane < LOCATE_WAVE; ++lane)
                if (chain_better(other_out[lane], other_pos[lane], best_out[lane], best_pos[lane])) { best_out[lane] = other_out[lane]; best_pos[lane] = other_pos[lane]; }
        }
        for (int lane = 1; lane < LOCATE_WAVE; ++lane)
            if (best_pos[lane] != best_pos[0] || best_out[lane] != best_out[0]) { st = -1; }      // the lanes must agree (never seen)
        if (st < 0) break;
        if (best_pos[0] == CHAIN_NONE || len >= count) { st = COVER_GAP; break; }
        chain_hit[first + len] = (int)(first + best_pos[0]);
        ++len;
        cur = best_out[0];
    }
    status[q] = st; reach[q] = cur; chain_len[q] = len;
}

template <int N>
static long long clip(int P, const int *ptr, const double *A, const double *b, int Q, const double *from, const double *to, double tol, long long *hit_ptr,
                      int *hit_region, unsigned char *hit_class, double *hit_in, double *hit_out, int *status, double *reach, long long *chain_ptr, int *chain_hit,
                      long long capacity)
{
    const LocateRegions R{P, ptr, A, b};
    const long long chunks = locate_chunks(P);
    const size_t cells = (size_t)(Q * chunks);
    std::vector<int> count(cells);
    std::vector<long long> offset(cells);
    std::vector<int64_t> hp((size_t)Q + 1, 0);
    for (long long q = 0; q < Q; ++q)
        for (long long c = 0; c < chunks; ++c)
            clip_block<N, false>(R, from, to, tol, chunks, 0, c, q, count.data(), nullptr, nullptr, nullptr, nullptr, nullptr);
    if (!locate_scan(count.data(), Q, chunks, offset.data(), hp.data())) return -1;
    const long long total = hp[(size_t)Q];
    std::vector<long long> hpl(hp.begin(), hp.end());
    if (hit_ptr)
        for (int q = 0; q <= Q; ++q) hit_ptr[q] = hpl[(size_t)q];
    if (total > capacity) return total;
    for (long long q = 0; q < Q; ++q)
        for (long long c = 0; c < chunks; ++c)
            clip_block<N, true>(R, from, to, tol, chunks, total, c, q, nullptr, offset.data(), hit_region, hit_class, hit_in, hit_out);
    // the chains at the segments' offsets, then packed as gcsadmm_scene_read_cover packs them
    std::vector<int> chain((size_t)total), len((size_t)Q);
    for (long long q = 0; q < Q; ++q) chain_block(hpl.data(), hit_in, hit_out, q, status, reach, len.data(), chain.data());
    long long at = 0;
    for (long long q = 0; q < Q; ++q) {
        chain_ptr[q] = at;
        std::copy_n(chain.begin() + hpl[(size_t)q], len[(size_t)q], chain_hit + at);
        at += len[(size_t)q];
    }
    chain_ptr[Q] = at;
    return total;
}

#define DIMS(call)                                                                                                                     \
    switch (n) {                                                                                                                       \
    case 1: return call(1); case 2: return call(2); case 3: return call(3); case 4: return call(4);                                    \
    case 5: return call(5); case 6: return call(6); case 7: return call(7); case 8: return call(8);                                    \
    }                                                                                                                                  \
    return -99;

// the whole call on the regions (ptr, A, b): returns the number of hits (-1: more than an int indexes), fills hit_ptr [Q + 1] and, when
// they have room for it (capacity entries each; chain_hit too: a chain is no longer than its segment's list), the list with its spans,
// status [Q], reach [Q], chain_ptr [Q + 1] and chain_hit
extern "C" long long clip_emu_call(int n, int P, const int *ptr, const double *A, const double *b, int Q, const double *from, const double *to, double tol,
                                   long long *hit_ptr, int *hit_region, unsigned char *hit_class, double *hit_in, double *hit_out, int *status, double *reach,
                                   long long *chain_ptr, int *chain_hit, long long capacity)
{
#define CALL(N) clip<N>(P, ptr, A, b, Q, from, to, tol, hit_ptr, hit_region, hit_class, hit_in, hit_out, status, reach, chain_ptr, chain_hit, capacity)
    DIMS(CALL)
#undef CALL
}

extern "C" int clip_emu_chunk(void) { return LOCATE_CHUNK; }

// ONE (segment, region) pair, straight from clip_direction and clip_span: what a plain double loop over segments and regions calls.
// Returns the class; a hit's span is filled
template <int N> static int pair(const int *ptr, const double *A, const double *b, int region, const double *p, const double *q, double tol, double *t_in, double *t_out)
{
    const LocateRegions R{region + 1, ptr, A, b};
    double d[N];
    clip_direction<N>(p, q, d);
    return clip_span<N>(R, region, p, d, tol, t_in, t_out);
}

extern "C" int clip_emu_pair(int n, const int *ptr, const double *A, const double *b, int region, const double *p, const double *q, double tol, double *t_in,
                             double *t_out)
{
#define CALL(N) pair<N>(ptr, A, b, region, p, q, tol, t_in, t_out)
    DIMS(CALL)
#undef CALL
}
