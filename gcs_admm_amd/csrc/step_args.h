// step_args.h -- the inputs every vertex-step program reads: the wavefront program (vertex_program.inc), the workgroup program
// (vertex_wg.h), the closed-form vertices (special_vertex.h) and the region terminals (terminal_region.h).  Their argument
// structs derive from StepArgs<T>; the host fills the untyped StepDesc once per launch (gcsadmm.hip make_step_graph / make_step).
// Host-compilable (the emulations in tests/hostemu and tools/flopcount include it): no hip_runtime.h.
#pragma once
#include <type_traits>

#include "gcs_math.h"

struct gcsadmm_control_block;

namespace gcsadmm_k {

constexpr int MAX_SPECIAL_DEG = 256;   // degree limit of the closed-form vertices (special_vertex.h): their work arrays are this long
constexpr int EDGE_BLOCK = 256;        // threads per workgroup of the edge kernel = edges the single-workgroup edge step holds
// FUSED TAIL (vertex_wg_kernel.h): LDS of the edge step the last workgroup of a vertex-step launch runs -- red[EDGE_BLOCK / 64][5] and
// the "came last" flag, in the dynamic segment the launch asks for
constexpr int FUSED_TAIL_LDS_BYTES = (EDGE_BLOCK / 64 * 5 + 1) * 8;
// dynamic LDS of a workgroup-program launch: the largest vertex of the plan, the work arrays of the closed-form workgroups, the tail
constexpr int wg_launch_lds_bytes(int plan_lds_bytes, bool fused_tail)
{
    int b = 4 * MAX_SPECIAL_DEG * 8;
    if (plan_lds_bytes > b) b = plan_lds_bytes;
    if (fused_tail && FUSED_TAIL_LDS_BYTES > b) b = FUSED_TAIL_LDS_BYTES;
    return b;
}

struct StepArgsBase {
    const int *inc_ptr;         // [V+1]
    const int *deg_in;          // [V]
    const int *inc_edge;        // [NI_owned]
    const int *poly_ptr;        // [V+1]
    const double *poly_A;       // [sum m][n]
    const double *poly_bc;      // [sum m] centred: b - A c
    const double *center;       // [V][n]
    int E, NI;
    int edge_major = 0;         // 1: state columns numbered by edge (tail side e, head side E + e) instead of by incidence
    double *xv, *zv, *yv;
    int *counters;              // [0] inner failures, [1] inner iterations
    double eps_edge, ipm_tol;
    int ipm_max_iter;
    // warm start (warm_start.h): the records of the handle's workspace, warm + warm_ptr[v]; nullptr = every solve starts cold
    double *warm = nullptr;
    const long long *warm_ptr = nullptr;
    // 1: the launch hands its copy columns to a reader in the SAME launch (the fused tail of vertex_wg_kernel): the solves store them
    // write-through (store_copy below).  Uniform over the launch; 0 everywhere else.
    int publish = 0;
};

// a word of the state's copy columns: a plain store, or for a publishing launch an agent-scope relaxed atomic store (sc1, write-through:
// it leaves the XCD's L2, so that an sc1 load of another workgroup of the launch finds it once the storing wavefront has drained)
template <class T> GCS_HD void store_copy(T *p, T v, int publish)
{
#if defined(__HIP_DEVICE_COMPILE__)
    if (publish) { __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); return; }
#endif
    (void)publish;
    *p = v;
}

// the state columns: zedge [2n+1][E], mu and copy [2n+1][NI], of the handle's state type (f64 / f32)
template <class T> struct StepArgs : StepArgsBase {
    const T *zedge, *mu;
    T *copy;
};

// host side: the same fields with the state untyped (the handle's dtype picks T at launch)
struct StepDesc : StepArgsBase {
    const void *zedge, *mu;
    void *copy;
    const gcsadmm_control_block *cb;
    template <class T> StepArgs<T> typed() const
    {
        StepArgs<T> a;
        static_cast<StepArgsBase &>(a) = *this;
        a.zedge = (const T *)zedge; a.mu = (const T *)mu; a.copy = (T *)copy;
        return a;
    }
};

// state column of local incidence k = lo + k of a vertex (edge id `edge`, outgoing or not): gcsadmm_graph_desc.edge_major_columns
GCS_HD int state_column(int edge_major, int E, int lo, int k, int edge, bool out) { return edge_major ? edge + (out ? 0 : E) : lo + k; }
// (A: StepArgs<T>, or a struct with the same field names -- gcs_term::TermProblem)
template <class A> GCS_HD int state_column(const A &a, int lo, int k, int edge, bool out) { return state_column(a.edge_major, a.E, lo, k, edge, out); }
// the same where the edge id is not loaded yet: edges[k] is read only when the columns are edge-major
template <class A> GCS_HD int state_column(const A &a, int lo, int k, const int *edges, bool out)
{
    return state_column(a.edge_major, a.E, lo, k, a.edge_major ? edges[k] : 0, out);
}

// consensus target of word w of an incidence: the edge's copy less the scaled dual of the incidence's state column
template <class A> GCS_HD double consensus_target(const A &a, int w, int edge, int col, double mu_scale)
{
    return (double)a.zedge[(size_t)w * a.E + edge] - mu_scale * (double)a.mu[(size_t)w * a.NI + col];
}

// f(std::integral_constant<int, N>()) for the N of Ns equal to n; false: n is none of them
template <int... Ns, class F> bool dispatch_dim(int n, F &&f)
{
    return ((n == Ns ? (f(std::integral_constant<int, Ns>()), true) : false) || ...);
}

// f(double()) or f(float()): the state type T of StepArgs<T>, chosen at run time (f64: the handle's dtype is GCSADMM_F64)
template <class F> auto with_state_type(bool f64, F &&f) { return f64 ? f(double()) : f(float()); }

}  // namespace gcsadmm_k
