// vertex_kernel.h -- device-side wrapper of the wavefront program (vertex_program.h): the kernel template,
// and the host-side launch helpers.  Instantiated for n = 2 (gcsadmm.hip); every other dimension, and every vertex the
// wavefront program cannot take, runs the workgroup program (vertex_wg.hip).
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>

#include "gcsadmm.h"
#include "special_vertex.h"
#include "vertex_program.h"

namespace gcsadmm_k {

using gcs::WAVE;

// everything a vertex-step launch of the wavefront program needs, as plain pointers (device) and scalars
struct VertexLaunchDesc {
    StepDesc step;
    int n_waves, n_special, all_m4, lds_bytes, align_rows, store_dl, MM;
    const int *wave_slot_ptr, *wave_vtx, *special_vtx, *special_kind;
    const int *wave_order;          // slowest-first dispatch (reorder_kernel): workgroup b runs wavefront wave_order[b]; may be null
    int *wave_iters;                // [n_waves] Newton iterations of each wavefront's last launch; may be null
};

#ifdef GCS_PHASE_TIMING
__device__ unsigned long long g_phase_cycles[64];
#endif

// RMODE: how the segmented reductions move data between lanes.  0 = DPP row shifts (host placed the groups so
// that no side segment straddles a 16-lane row), 1 = chained DPP wave_shl:1 (dense packing, segments may cross
// rows).  Either falls back to the ds_bpermute tree for a wavefront it cannot serve.  One mode per kernel
// instantiation: carrying both paths in one kernel costs ~4 % (code size).
template <class LaneT, int RMODE> struct GpuExec {
    LaneT &L;
    int lane;
#ifdef GCS_PHASE_TIMING
    // diagnostic build only: cycles per barrier-separated phase, summed over wavefronts
    int phase = 0;
    unsigned long long *acc;
    template <class F> __device__ __forceinline__ void each(F &&f)
    {
        const unsigned long long t0 = __builtin_amdgcn_s_memtime();
        f(L, lane);
        __syncthreads();
        const unsigned long long t1 = __builtin_amdgcn_s_memtime();
        if (lane == 0) acc[phase] += t1 - t0;
        phase = (phase == 13) ? 5 : phase + 1;   // 5 prologue phases, then 9 per Newton iteration (a cold repeat of a failed warm solve, rare, adds one)
    }
#else
    template <class F> __device__ __forceinline__ void each(F &&f)
    {
        f(L, lane);
        __syncthreads();
    }
#endif
    template <class P> __device__ __forceinline__ bool all(P &&p) { return __all(p(L) ? 1 : 0) != 0; }
    template <class F> __device__ __forceinline__ int wave_max(F &&f)
    {
        int m = f(L);
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) m = max(m, __shfl_xor(m, off, 64));
        return __builtin_amdgcn_readfirstlane(m);
    }
    // segmented reduction over the consecutive block lanes of one side of a vertex (vertex_program.inc):
    // shuffle-down tree, nsteps is wave-uniform; all 64 lanes execute it, non-contributors pass the identity.
    template <int SH> static __device__ __forceinline__ double row_down(double x)
    {
        // lane i reads lane i + SH of its 16-lane row (DPP row_shl); lanes past the row end read 0 and are masked off
        int lo = __double2loint(x), hi = __double2hiint(x);
        lo = __builtin_amdgcn_update_dpp(0, lo, 0x100 + SH, 0xf, 0xf, true);
        hi = __builtin_amdgcn_update_dpp(0, hi, 0x100 + SH, 0xf, 0xf, true);
        return __hiloint2double(hi, lo);
    }
    template <int SH> static __device__ __forceinline__ double wave_down(double x)
    {
        // lane i reads lane i + SH of the wavefront: SH chained DPP wave_shl:1 moves per half (lanes past 63 read 0)
        int lo = __double2loint(x), hi = __double2hiint(x);
#pragma unroll
        for (int k = 0; k < SH; ++k) {
            lo = __builtin_amdgcn_update_dpp(0, lo, 0x130, 0xf, 0xf, true);
            hi = __builtin_amdgcn_update_dpp(0, hi, 0x130, 0xf, 0xf, true);
        }
        return __hiloint2double(hi, lo);
    }
    template <int CNT, class SHUF>
    static __device__ __forceinline__ void seg_step(double (&v)[CNT], bool ok, int special, int op, SHUF &&shuf)
    {
#pragma unroll
        for (int k = 0; k < CNT; ++k) {
            const double t = shuf(v[k]);
            if (k == special && op == 1) v[k] = ok ? fmin(v[k], t) : v[k];
            else if (k == special && op == 2) v[k] = ok ? fmax(v[k], t) : v[k];
            else v[k] = ok ? v[k] + t : v[k];
        }
    }
    template <int CNT>
    __device__ __forceinline__ void seg_reduce(LaneT &L, double (&v)[CNT], double *sin, double *sout, int special, int op,
                                               bool contributes, int nsteps, bool rows)
    {
        if (RMODE == 0 && rows) {      // wave-uniform: segments never cross a 16-lane row, at most 4 steps
            if (nsteps > 0) seg_step<CNT>(v, (L.segmask >> 0) & 1, special, op, [](double x) { return row_down<1>(x); });
            if (nsteps > 1) seg_step<CNT>(v, (L.segmask >> 1) & 1, special, op, [](double x) { return row_down<2>(x); });
            if (nsteps > 2) seg_step<CNT>(v, (L.segmask >> 2) & 1, special, op, [](double x) { return row_down<4>(x); });
            if (nsteps > 3) seg_step<CNT>(v, (L.segmask >> 3) & 1, special, op, [](double x) { return row_down<8>(x); });
        } else if (RMODE == 1 && nsteps <= 3) {   // segments cross rows: whole-wave shifts by one lane (DPP wave_shl:1), chained
            if (nsteps > 0) seg_step<CNT>(v, (L.segmask >> 0) & 1, special, op, [](double x) { return wave_down<1>(x); });
            if (nsteps > 1) seg_step<CNT>(v, (L.segmask >> 1) & 1, special, op, [](double x) { return wave_down<2>(x); });
            if (nsteps > 2) seg_step<CNT>(v, (L.segmask >> 2) & 1, special, op, [](double x) { return wave_down<4>(x); });
        } else {
            for (int s = 0; s < nsteps; ++s)
                seg_step<CNT>(v, (L.segmask >> s) & 1, special, op, [s](double x) { return __shfl_down(x, 1 << s, 64); });
        }
        if (contributes && L.seg_head) {
            double *dst = L.out ? sout : sin;
#pragma unroll
            for (int k = 0; k < CNT; ++k) dst[k] = v[k];
        }
    }
    __device__ __forceinline__ void count(int *c, int fails, int iters)
    {
        if (fails) atomicAdd(&c[0], fails);
        atomicAdd(&c[1], iters);
    }
    __device__ __forceinline__ void note(int *p, int v) { if (lane == 0) *p = v; }      // one word per wavefront
};

// the two instantiations of the wavefront program (vertex_program.h); VertexLaunchDesc::all_m4 = 0 generic, 2 box
struct ProgGeneric {   // any facet count per polytope, facet-row duals in LDS
    template <int N> using LaneT = gcs::Lane<N>;
    template <class T> using Args = gcs::VertexArgs<T>;
    using Shared = gcs::WaveShared;
    static __device__ __forceinline__ void shared_init(Shared &S, double *smem, int n, int mm, int dl) { gcs::wave_shared_init(S, smem, n, mm, dl); }
    template <int N, class T, int SDL, class EX>
    static __device__ __forceinline__ void run(EX &ex, int w, const Args<T> &a, const Shared &S, double rho, double ms)
    {
        gcs::run_vertex_program<N, T, SDL>(ex, w, a, S, rho, ms);
    }
};
struct ProgBox {       // every polytope an axis-aligned box in canonical facet order (4 facets): unrolled facet loops, half of the row duals in registers, facet normals compile-time constants
    template <int N> using LaneT = gcs_box::Lane<N>;
    template <class T> using Args = gcs_box::VertexArgs<T>;
    using Shared = gcs_box::WaveShared;
    static __device__ __forceinline__ void shared_init(Shared &S, double *smem, int n, int mm, int dl) { gcs_box::wave_shared_init(S, smem, n, mm, dl); }
    template <int N, class T, int SDL, class EX>
    static __device__ __forceinline__ void run(EX &ex, int w, const Args<T> &a, const Shared &S, double rho, double ms)
    {
        gcs_box::run_vertex_program<N, T, SDL>(ex, w, a, S, rho, ms);
    }
};

// what one workgroup (one wavefront) of a vertex-step launch does once it knows its arguments: workgroup bx runs wavefront bx of the
// program (or wave_order[bx]), the trailing workgroups take the closed-form vertices.  One body for the kernel that gets its arguments
// in the kernarg segment (vertex_kernel) and the one that reads them from a table (vertex_wave_batch_kernel,
// vertex_wave_batch_kernel.h): the same instructions on the same numbers.
// SDL = 1: the LDS allocation has room for the final dual directions of the facet rows (lds_doubles(.., 1)); the
// update pass applies them instead of recomputing the rows.  Chosen by the host when it does not cost occupancy.
template <class PROG, int N, class T, int RMODE, int SDL>
__device__ __forceinline__ void vertex_wave_body(const typename PROG::template Args<T> &a, const SpecialArgs &sp, double rho, double mu_scale, int bx, double *smem)
{
    if (bx >= a.n_waves) {   // trailing workgroups: the special vertices, one per lane (saves a ~4 us launch per iteration)
        const int i = (bx - a.n_waves) * WAVE + (int)threadIdx.x;
        if (i < sp.count) {
            double *vals = smem + (sp.kind[i] == 2 ? 2 * MAX_SPECIAL_DEG : 0);   // source and target: own work arrays in LDS
            special_body<N, T>(a, sp, i, rho, mu_scale, vals, vals + MAX_SPECIAL_DEG);
        }
        return;
    }
    typename PROG::Shared S;
    PROG::shared_init(S, smem, N, a.MM, SDL);
    using LaneT = typename PROG::template LaneT<N>;
    LaneT L;
#ifdef GCS_PHASE_TIMING
    __shared__ unsigned long long acc[64];
    if (threadIdx.x < 64) acc[threadIdx.x] = 0;
    __syncthreads();
    GpuExec<LaneT, RMODE> ex{L, (int)threadIdx.x, 0, acc};
#else
    GpuExec<LaneT, RMODE> ex{L, (int)threadIdx.x};
#endif
    // (the launch ends when its slowest wavefront does: those that ran longest last time are dispatched first)
    PROG::template run<N, T, SDL>(ex, a.wave_order ? a.wave_order[bx] : bx, a, S, rho, mu_scale);
#ifdef GCS_PHASE_TIMING
    __syncthreads();
    if (threadIdx.x < 64) atomicAdd(&g_phase_cycles[threadIdx.x], acc[threadIdx.x]);
#endif
}

template <class PROG, int N, class T, int RMODE, int SDL>
__global__ __launch_bounds__(WAVE) void vertex_kernel(typename PROG::template Args<T> a, SpecialArgs sp, const gcsadmm_control_block *cb)
{
    extern __shared__ __attribute__((aligned(16))) double smem[];
    if (cb->status != GCSADMM_RUNNING) return;
    vertex_wave_body<PROG, N, T, RMODE, SDL>(a, sp, cb->rho, cb->mu_scale, (int)blockIdx.x, smem);
}

// The instantiations of the kernel, listed once: N = 2 (the tuned dimension) has PROG x RMODE x SDL -- dense packing + wave shifts, and
// the stored dual directions, exist for it only -- every other N the generic <0, 0> alone.  align_rows / store_dl: the plan's choices.
template <class PROG, int N, class T> using VertexKernelFn = void (*)(typename PROG::template Args<T>, SpecialArgs, const gcsadmm_control_block *);
template <class PROG, int N, class T> static VertexKernelFn<PROG, N, T> vertex_kernel_for(int align_rows, int store_dl)
{
    if constexpr (N == 2) {
        static const VertexKernelFn<PROG, N, T> by_rmode_sdl[2][2] = {{vertex_kernel<PROG, N, T, 0, 0>, vertex_kernel<PROG, N, T, 0, 1>},
                                                                      {vertex_kernel<PROG, N, T, 1, 0>, vertex_kernel<PROG, N, T, 1, 1>}};
        return by_rmode_sdl[align_rows ? 0 : 1][store_dl ? 1 : 0];
    } else {
        return vertex_kernel<PROG, N, T, 0, 0>;
    }
}
// vertex step for space dimension N: generic vertices (wavefront program) + special vertices (closed form)
template <int N, class T> static void launch_vertex_dim(const VertexLaunchDesc &d, hipStream_t s)
{
    if (d.n_waves + d.n_special <= 0) return;
    auto go = [&](auto prog) {
        using PROG = decltype(prog);
        typename PROG::template Args<T> a;
        static_cast<StepArgs<T> &>(a) = d.step.typed<T>();
        a.n_waves = d.n_waves; a.align_rows = d.align_rows; a.wave_slot_ptr = d.wave_slot_ptr; a.wave_vtx = d.wave_vtx; a.MM = d.MM;
        a.wave_order = d.wave_order; a.wave_iters = d.wave_iters;
        const SpecialArgs sp{d.n_special, d.special_vtx, d.special_kind};
        const unsigned grid = (unsigned)(d.n_waves + (d.n_special + WAVE - 1) / WAVE);
        const int lds = std::max(d.lds_bytes, (int)(4 * MAX_SPECIAL_DEG * sizeof(double)));   // room for the special work arrays
        hipLaunchKernelGGL((vertex_kernel_for<PROG, N, T>(d.align_rows, d.store_dl)), dim3(grid), dim3(WAVE), lds, s, a, sp, d.step.cb);
    };
    if (N != 2 || d.all_m4 != 2) go(ProgGeneric());
    else if constexpr (N == 2) go(ProgBox());     // the m = 4 program exists for n = 2 only
}

// raise the dynamic-LDS limit (needed above 48 KB) of every instantiation a handle with this all_m4 may launch
template <int N, class T> static hipError_t set_lds_attr(int all_m4, int lds_bytes)
{
    hipError_t e = hipSuccess;
    auto set_all = [&](auto prog) {
        for (int k = 0; k < (N == 2 ? 4 : 1) && e == hipSuccess; ++k)       // (RMODE, SDL) = (0, 0), (0, 1), (1, 0), (1, 1)
            e = hipFuncSetAttribute((const void *)vertex_kernel_for<decltype(prog), N, T>(k < 2, k & 1), hipFuncAttributeMaxDynamicSharedMemorySize, lds_bytes);
    };
    set_all(ProgGeneric());
    if constexpr (N == 2) {
        if (all_m4 == 2) set_all(ProgBox());
    }
    return e;
}

} // namespace gcsadmm_k

