// vertex_wave_batch_kernel.h -- BATCH form of the wavefront program (gcsadmm_batch_run on a batch made with GCSADMM_BATCH_LARGE): one
// launch serves the wavefront vertices of many handles.  It is to vertex_kernel (vertex_kernel.h) what vertex_wg_batch_kernel is to
// vertex_wg_kernel (vertex_wg_kernel.h): row blockIdx.y of the grid is member blockIdx.y of the launch's group, the workgroup -- one
// wavefront -- copies that member's entry of the table (the arguments vertex_kernel gets in its kernarg segment, the member's own
// control block and the width of its own grid) and runs vertex_wave_body on it.  The index is uniform over the wavefront, so the
// entry comes in through scalar loads and lives in scalar registers as kernel arguments do.  Wavefronts beyond the member's own grid
// (the launch is as wide as the widest member) and those of a member that has stopped leave at once, before any barrier or LDS use.
//
// Why a batch of these pays: the program takes the whole register file of a SIMD (one wavefront per SIMD, 1 024 slots on the chip), and
// a launch lasts as long as its slowest wavefront whether it fills 150 of those slots or 1 000.  A member packed at 4 to 7 vertices per
// wavefront leaves most of them empty; several members in one launch fill them.
//
// n = 2 only (the dimension the wavefront program is instantiated for): {generic, box} x {f64, f32} x RMODE x SDL, sixteen kernels.
// Like vertex_kernel.h this header holds the kernel template and its host-side launch helpers, and gcsadmm.hip instantiates it.  (The
// variant table of build.py rebuilds named units of the product and links every other one as it is; its tests pin those command
// lines, so the family has no object of its own.)
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>

#include "vertex_kernel.h"

namespace gcsadmm_k {

template <class PROG, class T> struct WaveBatchEntry {
    typename PROG::template Args<T> a;      // (wave_order null: a batch runs the wavefronts in index order)
    SpecialArgs sp;
    const gcsadmm_control_block *cb;
    int grid_x;                 // workgroups of this member: n_waves + ceil(n_special / 64)
};

template <class PROG, int N, class T, int RMODE, int SDL>
__global__ __launch_bounds__(WAVE) void vertex_wave_batch_kernel(const WaveBatchEntry<PROG, T> *__restrict__ table)
{
    static_assert(N == 2, "the wavefront program is tuned for, and batched at, n = 2");
    extern __shared__ __attribute__((aligned(16))) double smem[];
    // the table is written by the host before the launch and by nobody during it: it is read through the constant address space, as
    // kernel arguments are, so that the compiler may reload a field where it needs it instead of keeping all of them live
    using Entry = WaveBatchEntry<PROG, T>;
    __builtin_assume_dereferenceable(table + blockIdx.y, sizeof(Entry));
    const Entry e = *(const Entry *)((const __attribute__((address_space(4))) Entry *)table + blockIdx.y);
    if ((int)blockIdx.x >= e.grid_x || e.cb->status != GCSADMM_RUNNING) return;
    vertex_wave_body<PROG, N, T, RMODE, SDL>(e.a, e.sp, e.cb->rho, e.cb->mu_scale, (int)blockIdx.x, smem);
}

// one wave launch of a batch: `table` is a device array of `count` entries, one per member of the GROUP, laid out by wave_batch_fill.
// The members of a group share the three choices that select the instantiation.
struct WaveBatchLaunch {
    int dtype, all_m4, align_rows, store_dl;
    const void *table;
    unsigned grid_x, count;         // workgroups (wavefronts) of the widest member, members of the group
    int lds_bytes;                  // dynamic LDS of the largest member
};

// the instantiation a group runs, by the plan's choices (as vertex_kernel_for)
template <class PROG, class T> using WaveBatchKernelFn = void (*)(const WaveBatchEntry<PROG, T> *);
template <class PROG, class T> static WaveBatchKernelFn<PROG, T> wave_batch_kernel_for(int align_rows, int store_dl)
{
    static const WaveBatchKernelFn<PROG, T> by_rmode_sdl[2][2] = {{vertex_wave_batch_kernel<PROG, 2, T, 0, 0>, vertex_wave_batch_kernel<PROG, 2, T, 0, 1>},
                                                                  {vertex_wave_batch_kernel<PROG, 2, T, 1, 0>, vertex_wave_batch_kernel<PROG, 2, T, 1, 1>}};
    return by_rmode_sdl[align_rows ? 0 : 1][store_dl ? 1 : 0];
}

// f(ProgGeneric() or ProgBox(), double() or float()): the program and the state type of a launch (all_m4 = 2: box, as launch_vertex_dim)
template <class F> static auto with_wave_batch_types(int all_m4, int dtype, F &&f)
{
    return with_state_type(dtype == GCSADMM_F64, [&](auto t) {
        if (all_m4 == 2) return f(ProgBox(), t);
        return f(ProgGeneric(), t);
    });
}

// bytes of one table entry for that state type (the two programs' argument blocks have the same fields: one size per state type)
static size_t wave_batch_entry_bytes(int dtype)
{
    static_assert(sizeof(WaveBatchEntry<ProgGeneric, double>) == sizeof(WaveBatchEntry<ProgBox, double>), "one entry size per state type");
    static_assert(sizeof(WaveBatchEntry<ProgGeneric, float>) == sizeof(WaveBatchEntry<ProgBox, float>), "one entry size per state type");
    return dtype == GCSADMM_F64 ? sizeof(WaveBatchEntry<ProgGeneric, double>) : sizeof(WaveBatchEntry<ProgGeneric, float>);
}

// fill the entry at `entry_host` from the member's wave launch and its state type (d.step.cb is the member's control block;
// d.wave_order is ignored: a batch runs the wavefronts in index order); returns the width of the member's own grid, which the entry records
static int wave_batch_fill(const VertexLaunchDesc &d, int dtype, void *entry_host)
{
    const int grid_x = d.n_waves + (d.n_special + WAVE - 1) / WAVE;
    with_wave_batch_types(d.all_m4, dtype, [&](auto prog, auto t) {
        using PROG = decltype(prog);
        using T = decltype(t);
        typename PROG::template Args<T> a;
        static_cast<StepArgs<T> &>(a) = d.step.typed<T>();
        a.n_waves = d.n_waves; a.align_rows = d.align_rows; a.wave_slot_ptr = d.wave_slot_ptr; a.wave_vtx = d.wave_vtx; a.MM = d.MM;
        a.wave_order = nullptr; a.wave_iters = d.wave_iters;
        *(WaveBatchEntry<PROG, T> *)entry_host = WaveBatchEntry<PROG, T>{a, SpecialArgs{d.n_special, d.special_vtx, d.special_kind}, d.step.cb, grid_x};
    });
    return grid_x;
}

// raise the dynamic-LDS limit of the group's instantiation (needed above 48 KB), as set_lds_attr does for a solo handle
static hipError_t wave_batch_set_lds(const WaveBatchLaunch &b)
{
    return with_wave_batch_types(b.all_m4, b.dtype, [&](auto prog, auto t) {
        return hipFuncSetAttribute((const void *)wave_batch_kernel_for<decltype(prog), decltype(t)>(b.align_rows, b.store_dl),
                                   hipFuncAttributeMaxDynamicSharedMemorySize, b.lds_bytes);
    });
}

static void wave_batch_launch(const WaveBatchLaunch &b, hipStream_t s)
{
    if (b.grid_x == 0 || b.count == 0) return;
    const int lds = std::max(b.lds_bytes, (int)(4 * MAX_SPECIAL_DEG * sizeof(double)));      // room for the special work arrays
    with_wave_batch_types(b.all_m4, b.dtype, [&](auto prog, auto t) {
        using PROG = decltype(prog);
        using T = decltype(t);
        hipLaunchKernelGGL((wave_batch_kernel_for<PROG, T>(b.align_rows, b.store_dl)), dim3(b.grid_x, b.count), dim3(WAVE), lds, s,
                           (const WaveBatchEntry<PROG, T> *)b.table);
    });
}

}  // namespace gcsadmm_k
