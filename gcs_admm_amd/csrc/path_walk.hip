// path_walk.hip -- the candidate paths of the rounding step, drawn on the device (gfx950): walk_kernel and the gcsadmm_walks_* entry
// points.  path_walk_core.h has the rule.  The graphs of B problems are uploaded once; a call draws walks walk_first .. walk_first +
// num_walks - 1 of every problem, one 64-lane workgroup per (walk, problem), reading each problem's activations where the solver left
// them (a row of zedge), and returns the paths to the host: the only transfer is B * num_walks * max_len vertex ids.
#include <hip/hip_runtime.h>

#include <new>
#include <string>
#include <vector>

#include "gcsadmm.h"
#include "hip_owners.h"
#include "path_walk_core.h"

using namespace gcsadmm_walk;

// the calling thread's last failed create (gcsadmm_walks_last_error(NULL))
static thread_local std::string g_walk_err;

struct gcsadmm_walks_s {
    int B = 0, device = 0;
    long long max_vertices = 0;                           // of the largest problem: the bitmap of a launch
    std::vector<long long> edges;                         // E_i (host: nothing else is needed after create)
    DevBuf<long long> vertex_off, edge_off;               // the problems: offsets, CSR out-lists, terminals
    DevBuf<int> out_ptr, out_head, out_edge, src, dst;
    DevBuf<unsigned long long> y, seed;                   // per call (kept and grown): activation pointers, seeds,
    DevBuf<int> path_vtx, path_len, status;               //   results
    std::string err;
};

namespace {

struct WalkArgs {
    const long long *vertex_off, *edge_off;
    const int *out_ptr, *out_head, *out_edge, *src, *dst;
    const unsigned long long *y, *seed;
    int walk_first, num_walks, max_len;
    int *path_vtx, *path_len, *status;
};

// workgroup (walk, problem); dynamic LDS: the visited bitmap of the call's largest problem
template <class T> __global__ __launch_bounds__(WALK_WAVE) void walk_kernel(WalkArgs a)
{
    extern __shared__ uint32_t visited[];
    const int lane = threadIdx.x, p = blockIdx.y;
    const uint32_t walk = (uint32_t)a.walk_first + blockIdx.x;
    const long long v0 = a.vertex_off[p], e0 = a.edge_off[p];
    const int V = (int)(a.vertex_off[p + 1] - v0);
    const int *out_ptr = a.out_ptr + v0 + p, *out_head = a.out_head + e0, *out_edge = a.out_edge + e0;
    const T *y = (const T *)a.y[p];
    const uint64_t seed = a.seed[p];
    const size_t slot = (size_t)p * a.num_walks + blockIdx.x;
    int *path = a.path_vtx + slot * a.max_len;

    for (int i = lane; i < (V + 31) / 32; i += WALK_WAVE) visited[i] = 0;
    __syncthreads();
    int cur = a.src[p], len = 1, status = WALK_OK;
    const int dst = a.dst[p];
    if (lane == 0) { path[0] = cur; walk_visit(visited, cur); }
    __syncthreads();
    while (cur != dst) {
        const int begin = out_ptr[cur], end = out_ptr[cur + 1];
        uint64_t sum = 0, best_w = 0;
        int best_k = -1;
        for (int base = begin; base < end; base += WALK_WAVE) {
            const WalkItem it = walk_item<T>(out_head, out_edge, y, visited, base + lane, end);
            sum += it.w;
            if (it.w > 0 && walk_better(it.w, base + lane, best_w, best_k)) { best_w = it.w; best_k = base + lane; }
        }
        const uint64_t tot = walk_wave_sum(sum);
        if (tot == 0) { status = WALK_DEAD_END; break; }
        if (len == a.max_len) { status = WALK_TOO_LONG; break; }
        int pick = -1;
        if (walk == 0) {
            walk_wave_max(best_w, best_k);
            pick = best_k;
        } else {
            const uint64_t r = walk_mulhi(walk_mix(seed, walk, (uint32_t)(len - 1)), tot);
            uint64_t before = 0;
            for (int base = begin; base < end && pick < 0; base += WALK_WAVE) {
                const WalkItem it = walk_item<T>(out_head, out_edge, y, visited, base + lane, end);
                const uint64_t inclusive = before + walk_wave_scan(it.w, lane);
                const int at = walk_wave_pick(inclusive, r);
                if (at >= 0) pick = base + at;
                before = __shfl((unsigned long long)inclusive, WALK_WAVE - 1, WALK_WAVE);
            }
        }
        if (pick < 0) { status = WALK_DEAD_END; break; }      // (r < tot: some prefix sum exceeds it)
        cur = out_head[pick];
        if (lane == 0) { path[len] = cur; walk_visit(visited, cur); }
        ++len;
        __syncthreads();
    }
    if (lane == 0) { a.path_len[slot] = len; a.status[slot] = status; }
}

int fail(gcsadmm_walks_s *w, int rc, std::string text)
{
    (w ? w->err : g_walk_err) = std::move(text);
    return rc;
}
#define WALKCHK(w, call)                                                                             \
    do {                                                                                             \
        hipError_t e_ = (call);                                                                      \
        if (e_ != hipSuccess) return fail(w, GCSADMM_ERR_HIP, std::string(#call) + ": " + hipGetErrorString(e_)); \
    } while (0)

template <class T> hipError_t reserve(DevBuf<T> &buf, size_t count) { return buf.size() >= count && buf ? hipSuccess : buf.alloc(count); }

int walks_create(int B, const int64_t *vertex_off, const int64_t *edge_off, const int *out_ptr, const int *out_head, const int *out_edge,
                 const int *src, const int *dst, int device, gcsadmm_walks_s **out)
{
    if (!out) return fail(nullptr, GCSADMM_ERR_BAD_ARG, "null out");
    *out = nullptr;
    if (B < 0 || !vertex_off || !edge_off || (B > 0 && (!out_ptr || !out_head || !out_edge || !src || !dst)))
        return fail(nullptr, GCSADMM_ERR_BAD_ARG, "negative number of problems or null array");
    if (vertex_off[0] != 0 || edge_off[0] != 0) return fail(nullptr, GCSADMM_ERR_BAD_ARG, "vertex_off[0] and edge_off[0] must be 0");
    std::vector<long long> voff((size_t)B + 1), eoff((size_t)B + 1), edges((size_t)B);
    long long max_vertices = 0;
    for (int i = 0; i <= B; ++i) { voff[(size_t)i] = vertex_off[i]; eoff[(size_t)i] = edge_off[i]; }
    for (int i = 0; i < B; ++i) {
        const long long V = voff[(size_t)i + 1] - voff[(size_t)i], E = eoff[(size_t)i + 1] - eoff[(size_t)i];
        const char *why = nullptr;
        long long at = -1;
        // (the limit on V first: nothing of an oversized or negative-sized problem is read)
        const int rc = walk_check_problem(V, E, out_ptr + voff[(size_t)i] + i, out_head + eoff[(size_t)i], out_edge + eoff[(size_t)i],
                                          V >= 1 ? src[i] : 0, V >= 1 ? dst[i] : 0, why, at);
        if (rc) return fail(nullptr, rc, "problem " + std::to_string(i) + ": " + why + (at >= 0 ? " " + std::to_string(at) : ""));
        edges[(size_t)i] = E;
        max_vertices = V > max_vertices ? V : max_vertices;
    }
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) return fail(nullptr, GCSADMM_ERR_NO_DEVICE, "no HIP device");
    if (device < 0 || device >= ndev) return fail(nullptr, GCSADMM_ERR_BAD_ARG, "device ordinal out of range");
    DeviceGuard guard(device);
    if (guard.err != hipSuccess) return fail(nullptr, GCSADMM_ERR_HIP, std::string("hipSetDevice: ") + hipGetErrorString(guard.err));
    std::unique_ptr<gcsadmm_walks_s> w(new gcsadmm_walks_s);      // (released under the guard on a failed upload)
    w->B = B; w->device = device; w->max_vertices = max_vertices; w->edges.swap(edges);
    const size_t nv = (size_t)voff[(size_t)B], ne = (size_t)eoff[(size_t)B];
    WALKCHK(nullptr, w->vertex_off.upload(voff.data(), voff.size()));
    WALKCHK(nullptr, w->edge_off.upload(eoff.data(), eoff.size()));
    if (B > 0) {
        WALKCHK(nullptr, w->out_ptr.upload(out_ptr, nv + (size_t)B));
        WALKCHK(nullptr, w->src.upload(src, (size_t)B));
        WALKCHK(nullptr, w->dst.upload(dst, (size_t)B));
    }
    if (ne > 0) {
        WALKCHK(nullptr, w->out_head.upload(out_head, ne));
        WALKCHK(nullptr, w->out_edge.upload(out_edge, ne));
    }
    *out = w.release();
    return GCSADMM_OK;
}

int walks_sample(gcsadmm_walks_s *w, const void *const *y_dev, int state_dtype, const int64_t *seed, int walk_first, int num_walks, int max_len,
                 hipStream_t stream, int *path_vtx, int *path_len, int *status)
{
    if (state_dtype != GCSADMM_F64 && state_dtype != GCSADMM_F32) return fail(w, GCSADMM_ERR_BAD_ARG, "state_dtype must be GCSADMM_F64 or GCSADMM_F32");
    if (walk_first < 0 || num_walks < 0 || (long long)walk_first + num_walks > (long long)INT32_MAX)
        return fail(w, GCSADMM_ERR_BAD_ARG, "walk_first and num_walks must be non-negative (and their sum an int)");
    if (max_len < 1) return fail(w, GCSADMM_ERR_BAD_ARG, "max_len must be at least 1");
    const long long slots = (long long)w->B * num_walks;
    if (slots == 0) return GCSADMM_OK;
    if (w->B > 65535) return fail(w, GCSADMM_ERR_UNSUPPORTED, "more than 65535 problems in one call");
    if (slots * max_len > (long long)INT32_MAX) return fail(w, GCSADMM_ERR_UNSUPPORTED, "num_problems * num_walks * max_len above 2^31 - 1");
    if (!y_dev || !seed || !path_vtx || !path_len || !status) return fail(w, GCSADMM_ERR_BAD_ARG, "null array");
    std::vector<unsigned long long> y((size_t)w->B), sd((size_t)w->B);
    for (int i = 0; i < w->B; ++i) {
        if (!y_dev[i] && w->edges[(size_t)i] > 0) return fail(w, GCSADMM_ERR_BAD_ARG, "problem " + std::to_string(i) + ": null activations");
        y[(size_t)i] = (unsigned long long)(uintptr_t)y_dev[i];
        sd[(size_t)i] = (unsigned long long)seed[i];
    }
    const size_t B = (size_t)w->B, cells = (size_t)(slots * max_len);
    WALKCHK(w, reserve(w->y, B)); WALKCHK(w, reserve(w->seed, B));
    WALKCHK(w, reserve(w->path_vtx, cells)); WALKCHK(w, reserve(w->path_len, (size_t)slots)); WALKCHK(w, reserve(w->status, (size_t)slots));
    WALKCHK(w, hipMemcpyAsync(w->y.get(), y.data(), sizeof(unsigned long long) * B, hipMemcpyHostToDevice, stream));
    WALKCHK(w, hipMemcpyAsync(w->seed.get(), sd.data(), sizeof(unsigned long long) * B, hipMemcpyHostToDevice, stream));
    const WalkArgs a{w->vertex_off.get(), w->edge_off.get(), w->out_ptr.get(), w->out_head.get(), w->out_edge.get(), w->src.get(), w->dst.get(),
                     w->y.get(), w->seed.get(), walk_first, num_walks, max_len, w->path_vtx.get(), w->path_len.get(), w->status.get()};
    const size_t lds = walk_bitmap_words(w->max_vertices) * sizeof(uint32_t);
    const dim3 grid((unsigned)num_walks, (unsigned)w->B);
    if (state_dtype == GCSADMM_F64) hipLaunchKernelGGL(walk_kernel<double>, grid, dim3(WALK_WAVE), lds, stream, a);
    else hipLaunchKernelGGL(walk_kernel<float>, grid, dim3(WALK_WAVE), lds, stream, a);
    WALKCHK(w, hipGetLastError());
    WALKCHK(w, hipMemcpyAsync(path_vtx, w->path_vtx.get(), sizeof(int) * cells, hipMemcpyDeviceToHost, stream));
    WALKCHK(w, hipMemcpyAsync(path_len, w->path_len.get(), sizeof(int) * (size_t)slots, hipMemcpyDeviceToHost, stream));
    WALKCHK(w, hipMemcpyAsync(status, w->status.get(), sizeof(int) * (size_t)slots, hipMemcpyDeviceToHost, stream));
    WALKCHK(w, hipStreamSynchronize(stream));
    return GCSADMM_OK;
}

} // namespace

extern "C" {

int gcsadmm_walks_create(int num_problems, const int64_t *vertex_off, const int64_t *edge_off, const int *out_ptr, const int *out_head,
                         const int *out_edge, const int *src, const int *dst, int device, struct gcsadmm_walks_s **out)
{
    try {
        return walks_create(num_problems, vertex_off, edge_off, out_ptr, out_head, out_edge, src, dst, device, out);
    } catch (const std::bad_alloc &) {
        return fail(nullptr, GCSADMM_ERR_NO_MEMORY, "out of host memory");
    }
}

void gcsadmm_walks_destroy(struct gcsadmm_walks_s *w)
{
    if (!w) return;
    DeviceGuard device_guard_(w->device);
    delete w;
}

const char *gcsadmm_walks_last_error(struct gcsadmm_walks_s *w) { return (w ? w->err : g_walk_err).c_str(); }

int gcsadmm_walks_sample(struct gcsadmm_walks_s *w, const void *const *y_dev, int state_dtype, const int64_t *seed, int walk_first,
                         int num_walks, int max_len, void *stream, int *path_vtx, int *path_len, int *status)
{
    if (!w) return fail(nullptr, GCSADMM_ERR_BAD_ARG, "null walks object");
    DeviceGuard device_guard_(w->device);
    if (device_guard_.err != hipSuccess) return fail(w, GCSADMM_ERR_HIP, std::string("hipSetDevice: ") + hipGetErrorString(device_guard_.err));
    try {
        return walks_sample(w, y_dev, state_dtype, seed, walk_first, num_walks, max_len, (hipStream_t)stream, path_vtx, path_len, status);
    } catch (const std::bad_alloc &) {
        return fail(w, GCSADMM_ERR_NO_MEMORY, "out of host memory");
    }
}

} // extern "C"
