// Host build of walk_kernel of csrc/path_walk.hip (path_walk_core.h): one workgroup's walk with the 64 lanes run one after the other,
// the stride's total, scan, ballot and maximum formed from their 64 values.  Test infrastructure: never shipped, never timed.
#include <vector>
#include "path_walk_core.h"
using namespace gcsadmm_walk;

// walk_kernel<T> for workgroup (walk, problem) of a one-problem call
template <class T>
static void walk_block(int V, const int *out_ptr, const int *out_head, const int *out_edge, const T *y, int src, int dst, uint64_t seed, uint32_t walk,
                       int max_len, int *path, int *path_len, int *status_out)
{
    std::vector<uint32_t> visited(walk_bitmap_words(V), 0u);
    int cur = src, len = 1, status = WALK_OK;
    path[0] = cur; walk_visit(visited.data(), cur);
    while (cur != dst) {
        const int begin = out_ptr[cur], end = out_ptr[cur + 1];
        uint64_t sum[WALK_WAVE] = {}, best_w[WALK_WAVE] = {};
        int best_k[WALK_WAVE];
        for (int lane = 0; lane < WALK_WAVE; ++lane) best_k[lane] = -1;
        for (int base = begin; base < end; base += WALK_WAVE)
            for (int lane = 0; lane < WALK_WAVE; ++lane) {
                const WalkItem it = walk_item<T>(out_head, out_edge, y, visited.data(), base + lane, end);
                sum[lane] += it.w;
                if (it.w > 0 && walk_better(it.w, base + lane, best_w[lane], best_k[lane])) { best_w[lane] = it.w; best_k[lane] = base + lane; }
            }
        const uint64_t tot = walk_wave_sum(sum);
        if (tot == 0) { status = WALK_DEAD_END; break; }
        if (len == max_len) { status = WALK_TOO_LONG; break; }
        int pick = -1;
        if (walk == 0) {
            uint64_t w;
            walk_wave_max(best_w, best_k, w, pick);
        } else {
            const uint64_t r = walk_mulhi(walk_mix(seed, walk, (uint32_t)(len - 1)), tot);
            uint64_t before = 0;
            for (int base = begin; base < end && pick < 0; base += WALK_WAVE) {
                uint64_t w[WALK_WAVE], inclusive[WALK_WAVE];
                for (int lane = 0; lane < WALK_WAVE; ++lane) w[lane] = walk_item<T>(out_head, out_edge, y, visited.data(), base + lane, end).w;
                walk_wave_scan(w, inclusive);
                for (int lane = 0; lane < WALK_WAVE; ++lane) inclusive[lane] += before;
                const int at = walk_wave_pick(inclusive, r);
                if (at >= 0) pick = base + at;
                before = inclusive[WALK_WAVE - 1];
            }
        }
        if (pick < 0) { status = WALK_DEAD_END; break; }
        cur = out_head[pick];
        path[len] = cur; walk_visit(visited.data(), cur);
        ++len;
    }
    *path_len = len; *status_out = status;
}

// walks walk_first .. walk_first + num_walks - 1 of one problem: path_vtx[num_walks][max_len], path_len / status [num_walks].  Returns what
// walk_check_problem returns for the problem (0: walked)
extern "C" int walk_emu_sample(int V, int E, const int *out_ptr, const int *out_head, const int *out_edge, const void *y, int is_f32, int src, int dst,
                               unsigned long long seed, int walk_first, int num_walks, int max_len, int *path_vtx, int *path_len, int *status)
{
    const char *why = nullptr;
    long long at = -1;
    if (const int rc = walk_check_problem(V, E, out_ptr, out_head, out_edge, src, dst, why, at)) return rc;
    if (max_len < 1) return 1;
    for (int i = 0; i < num_walks; ++i) {
        int *path = path_vtx + (size_t)i * max_len;
        if (is_f32) walk_block<float>(V, out_ptr, out_head, out_edge, (const float *)y, src, dst, seed, (uint32_t)(walk_first + i), max_len, path, path_len + i, status + i);
        else walk_block<double>(V, out_ptr, out_head, out_edge, (const double *)y, src, dst, seed, (uint32_t)(walk_first + i), max_len, path, path_len + i, status + i);
    }
    return 0;
}

// the pieces by themselves
extern "C" unsigned long long walk_emu_weight(double y) { return walk_weight(y); }
extern "C" unsigned long long walk_emu_mix(unsigned long long seed, unsigned walk, unsigned j) { return walk_mix(seed, walk, j); }
extern "C" unsigned long long walk_emu_mulhi(unsigned long long a, unsigned long long b) { return walk_mulhi(a, b); }
