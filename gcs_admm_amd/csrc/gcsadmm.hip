// gcsadmm.hip -- C ABI (include/gcsadmm.h) of the ADMM iteration loop: the handle and batch structs, the launch descriptors and
// helpers, the entry points.  Its kernels are in loop_kernels.h, the RCCL binding in rccl_api.h, the host-only rules of a vertex
// partition in halo_plan.h (as those of create and of a batch are in create_plan.h and batch_plan.h).
//
// Kernels of the loop (one HIP stream, launched back to back, no host round trip inside the loop):
//   vertex_kernel<2,T>   x-update, wavefront program (n = 2, degree <= 63): one wavefront per workgroup, several vertices
//                        per wavefront, program in vertex_program.inc   (admm_solver_v3.py:352-540)
//   vertex_wg_kernel<N,T> (vertex_wg.hip) x-update, workgroup program: one 256-thread workgroup per vertex, any n / degree
//                        trailing workgroups of either launch: x-update of s, t (closed form) and of vertices no flow can cross
//   vertex_wg_split_kernel<N,T> (vertex_wg.hip) the same program for vertices too large for LDS, edge blocks in a device workspace
//   edge_kernel<T,MODE,C> z-update, dual update, five partial norms     (admm_solver_v3.py:543-614); in gcsadmm_run the last
//                        workgroup to finish also does the final reduction and the control step (one launch per edge step)
//   finalize_kernel / control_kernel   deterministic final reduction; residuals, rho adaptation, stop test,
//                        trace record (admm_solver_v3.py:697-733): the separate steps of the partitioned loop
//   halo_pack / halo_unpack_kernel     messages of the cut edges' copies between vertex partitions (RCCL); in the overlapped
//                        partitioned loop they and the transfer run on a second stream while the interior wavefronts are solved
//   cost_kernel<T>       GCS_utils.py:184-211
//   vertex_wg_batch_kernel<N,T> (vertex_wg.hip) / edge_batch_kernel<T,C> / batch_poll_kernel   the loop of a BATCH of handles
//                        (gcsadmm_batch_run): the bodies of vertex_wg_kernel and edge_kernel on the member blockIdx.y names, each member
//                        with its own arguments and control state, one vertex launch and one edge + control launch per iteration
//   vertex_wave_batch_kernel<PROG,2,T,RMODE,SDL> (vertex_wave_batch_kernel.h)   the same for vertex_kernel, in batches made with
//                        GCSADMM_BATCH_LARGE: one launch per group of members that run the same instantiation
//   terminal_region_batch_kernel<N,T,LDSWS> (terminal_region.hip)   the same for terminal_region_kernel, in batches made with
//                        GCSADMM_BATCH_TERMINALS: one launch per group of terminals, on the batch's auxiliary stream
//   state_export_kernel<T> / state_import_kernel<T> (state_transfer_core.h)   replanning: the state of a solved handle written to a snapshot
//                        keyed by stable vertex ids, and read into the state of another graph of the scene; all members of a call in one launch
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <memory>
#include <new>
#include <string>
#include <type_traits>
#include <vector>

#include "gcsadmm.h"
#include "hip_owners.h"
#include "terminal_launch.h"
#ifdef GCS_PHASE_TIMING
// diagnostic build: sub-phase stamps inside the border factorisation (lane 0 of each wavefront)
__device__ unsigned long long g_sub_cycles[16];
__device__ __forceinline__ void gcs_stamp(int k)
{
    static __shared__ unsigned long long last;
    __builtin_amdgcn_sched_barrier(0);
    if (threadIdx.x == 0) {
        const unsigned long long t = __builtin_amdgcn_s_memtime();
        if (k > 0) atomicAdd(&g_sub_cycles[k], t - last);
        last = t;
    }
    __builtin_amdgcn_sched_barrier(0);
}
#define GCS_STAMP(k) gcs_stamp(k)
#endif
#include "vertex_kernel.h"
#include "vertex_wave_batch_kernel.h"
#include "vertex_wg_launch.h"
#include "warm_start.h"
#include "canonical_box.h"
#include "create_plan.h"
#include "batch_plan.h"
#include "edge_step.h"
#include "halo_plan.h"
#include "loop_kernels.h"
#include "rccl_api.h"

// =================================================================================================
// host side
// =================================================================================================
// (the owners of the device resources -- DevBuf<T>, Stream, Event -- and the DeviceGuard: hip_owners.h)
// vertex partition across GPUs (gcsadmm_attach_comm): the halo lists and the message layout (halo_plan.h) with what is uploaded of them
struct Halo : HaloPlan {
    DevBuf<int> d_send_cols, d_send_base, d_send_stride, d_recv_cols, d_recv_base, d_recv_stride;
    DevBuf<char> d_sendbuf, d_recvbuf;
    DevBuf<double> d_sums6;           // the five norms + the inner-failure count, all-reduced together
    bool attached() const { return (bool)d_sums6; }
};
// overlapped partitioned loop (boundary vertices first, the halo exchange behind them while the interior is solved): the
// split of the wavefronts into boundary (holding a vertex with a cut edge) and interior, a second stream for the exchange and two events
struct Overlap {
    int n_wave_b = 0;         // boundary wavefronts (0: no split)
    DevBuf<int> d_split_ids, d_split_order;    // [n_waves] static ids / launch order: boundary wavefronts first, then interior
    Stream comm_stream;
    Event ev_boundary, ev_halo;
};
// terminals that are regions (terminal_region.h): at most two, one workgroup each, on an auxiliary stream beside the vertex-step launch
struct Terminals {
    DevBuf<double> d_term_ws, d_term_rec;      // work arrays (when they do not fit LDS); warm-start records
    Stream term_stream;
    Event ev_term_fork, ev_term_join;
};

// The decisions of create are the plan's (create_plan.h), kept as made; the handle adds the descriptor's scalars, the run state and
// the owners of what lives on the device, grouped by lifetime.
struct gcsadmm_handle_s {
    int n = 0, V = 0, E = 0, NI = 0, c = 0, dtype = 0, device = 0, src = -1, dst = -1;
    int edge_major = 0;       // state columns numbered by edge (gcsadmm_graph_desc.edge_major_columns)
    CreatePlan plan;          // (its arrays that only fed an upload are released after it: the buffers below know their lengths)
    gcsadmm_params params{};
    bool params_set = false;
    int vertex_steps = 0;     // vertex steps enqueued since the last reset
    unsigned resets = 0;      // gcsadmm_reset calls: a batch's tables hold what the reset before its bind set (gcsadmm_batch_run compares)
    gcsadmm_batch_s *batch = nullptr;      // the batch this handle is bound to (gcsadmm_batch_bind .. the batch's next bind or its destroy)
    std::vector<gcsadmm_batch_s *> batches;      // the batches that list this handle as a member (gcsadmm_batch_create .. _destroy)
    int overlap_mode = 0;     // gcsadmm_set_overlap: 0 automatic, 1 forced (tests: works without peers), 2 off
    int fused_tail_mode = 1;  // gcsadmm_set_fused_tail: 0 two launches per iteration, 1 automatic (one where the plan allows it)
    std::string err;
    void *comm = nullptr;     // ncclComm_t (gcsadmm_attach_comm)
    int rank = 0, world = 1;
    std::vector<int> iota;    // 0, 1, ..: the initial launch order of the slowest-first dispatch (create and every reset upload it)
    // the graph and what the plan made of it: from create to destroy
    struct Graph {
        DevBuf<int> d_inc_ptr, d_deg_in, d_inc_edge, d_poly_ptr, d_edge_inc_tail, d_edge_inc_head;
        DevBuf<int> d_edge_tail, d_edge_head;      // both ends of every edge as vertices (plan.edge_tail / edge_head), uploaded by the first
                                                   // state transfer of the handle: create allocates what it always did
        DevBuf<int> d_wave_slot_ptr, d_wave_vtx, d_special_vtx, d_special_kind, d_wg_vtx;
        DevBuf<double> d_poly_A, d_poly_bc, d_center;
        DevBuf<uint8_t> d_inc_counted, d_edge_counted;      // may stay empty
        // split form of the workgroup program (gcsadmm_graph_desc.vertex_workspace): vertices, their units' slabs
        DevBuf<int> d_split_vtx;
        DevBuf<long long> d_split_off;
        DevBuf<double> d_split_ws;
        // warm start of the vertex solves (warm_start.h): one record per generic vertex, d_warm + d_warm_ptr[v]
        DevBuf<double> d_warm;
        DevBuf<long long> d_warm_ptr;
        // slowest-first dispatch (reorder_kernel): per wavefront / per workgroup-program vertex, last Newton iteration count and launch order
        DevBuf<int> d_wave_iters, d_wave_order, d_wg_iters, d_wg_order;
    } g;
    // scratch of the iteration loop
    struct Loop {
        DevBuf<gcsadmm_control_block> d_cb;
        DevBuf<int> d_counters;
        DevBuf<double> d_partials, d_sums;
        DevBuf<unsigned> d_ticket;      // arrival counter of the single-launch edge step (edge_kernel MODE 2)
        DevBuf<char> d_transfer;        // table and vertex ids of the last gcsadmm_export_state / gcsadmm_import_state (grows, is kept)
    } loop;
    struct Prox { DevBuf<int> d_prox_vtx, d_prox_counters; } prox;      // gcsadmm_vertex_prox: every non-terminal vertex, own counters
    Halo halo;
    Overlap overlap;
    Terminals term;
    std::vector<Event> events;      // pool of timing events (gcsadmm_run_timed, gcsadmm_run_partitioned_timed)

    int n_special() const { return (int)g.d_special_vtx.size(); }
    int n_wg() const { return (int)g.d_wg_vtx.size(); }       // vertices solved by the workgroup program (vertex_wg.hip)
    int n_split() const { return (int)g.d_split_vtx.size(); }
    // gcsadmm_run runs the edge and control steps as the tail of the vertex launch (a handle attached to a communicator does not)
    bool fuses() const { return plan.fused_tail && fused_tail_mode != 0 && !halo.attached(); }
};

// A batch of handles (gcsadmm_batch_create): the members stay the caller's, the batch owns its plan (batch_plan.h) and the argument
// tables of its two kernels.  Nothing of a member's loop state moves: the entries point at the members' own control blocks, counters,
// partials, sums and tickets, which is why a member run in a batch and the same handle run alone produce the same bits.
struct gcsadmm_batch_s {
    int device = 0;
    std::string err;
    std::vector<gcsadmm_handle> members;
    std::vector<unsigned> resets;       // members' reset counts at bind
    std::vector<gcsadmm_state> states;  // members' state pointers at bind (gcsadmm_batch_export_state / _import_state work on them)
    DevBuf<char> d_transfer;            // table and vertex ids of the last of those calls (grows, is kept)
    BatchPlan plan;
    bool bound = false;
    unsigned flags = 0;                 // GCSADMM_BATCH_LARGE | GCSADMM_BATCH_TERMINALS or 0 (gcsadmm_batch_create_ex)
    DevBuf<char> d_vertex_table, d_edge_table;      // [plan.wg_members.size()] WgBatchEntry<T> (vertex_wg_launch.h) / [count] EdgeBatchEntry<T>
    DevBuf<char> d_wave_table;                      // the groups' tables back to back, each [members of the group] WaveBatchEntry<PROG, T> (vertex_wave_batch_kernel.h)
    DevBuf<const gcsadmm_control_block *> d_cbs;    // [count] the members' control blocks (batch_poll_kernel)
    DevBuf<int> d_poll;                             // [2 count] status, it
    // GCSADMM_BATCH_TERMINALS: the groups' tables back to back, each [terminals of the group] TermBatchEntry<T> (terminal_launch.h); the
    // batch's own auxiliary stream for their launches beside the vertex launches, as Terminals has for a solo handle
    DevBuf<char> d_term_table;
    Stream term_stream;
    Event ev_term_fork, ev_term_join;
    std::vector<int> poll_host;
};


static thread_local std::string g_create_error;      // gcsadmm_last_error(NULL): the calling thread's last failed create

// of one family with NCCLCHK (rccl_api.h): `obj` is the handle or batch whose err takes the text
#define HIPCHK(obj, call)                                                                            \
    do {                                                                                             \
        hipError_t e_ = (call);                                                                      \
        if (e_ != hipSuccess) {                                                                      \
            (obj)->err = std::string(#call) + ": " + hipGetErrorString(e_);                          \
            return GCSADMM_ERR_HIP;                                                                  \
        }                                                                                            \
    } while (0)

// The one shim of the entry points: no exception crosses the C ABI, a failed host allocation (a plan, a table, an event of the pool,
// the text of a refusal) is a status.  `err` takes its text: the object's, or g_create_error for the calls without one.
template <class F> static gcsadmm_status entry(std::string &err, F &&body)
{
    try {
        return body();
    } catch (const std::bad_alloc &) {
        try { err = "out of host memory"; } catch (...) { err.clear(); }
        return GCSADMM_ERR_NO_MEMORY;
    }
}
// ... of every call on a handle or a batch that reaches the device: a null object is refused, `args` checks the other arguments on the
// host, then the object's device is held for `body` and the caller's is back on return (DeviceGuard, hip_owners.h)
template <class O, class A, class F> static gcsadmm_status guarded_entry(O *obj, A &&args, F &&body)
{
    if (!obj) return GCSADMM_ERR_BAD_ARG;
    return entry(obj->err, [&]() -> gcsadmm_status {
        const gcsadmm_status refused = args();
        if (refused != GCSADMM_OK) return refused;
        DeviceGuard device_guard_(obj->device);
        if (device_guard_.err != hipSuccess) { obj->err = std::string("hipSetDevice: ") + hipGetErrorString(device_guard_.err); return GCSADMM_ERR_HIP; }
        return body();
    });
}
template <class A, class F> static gcsadmm_status handle_entry(gcsadmm_handle h, A &&args, F &&body) { return guarded_entry(h, args, body); }
template <class A, class F> static gcsadmm_status batch_entry(gcsadmm_batch_s *b, A &&args, F &&body) { return guarded_entry(b, args, body); }
static gcsadmm_status bad_unless(bool ok) { return ok ? GCSADMM_OK : GCSADMM_ERR_BAD_ARG; }

// f(double()) or f(float()): the one switch on the handle's state type
template <class F> static auto with_state(const gcsadmm_handle_s *h, F &&f) { return with_state_type(h->dtype == GCSADMM_F64, f); }
static size_t state_bytes(const gcsadmm_handle_s *h) { return h->dtype == GCSADMM_F64 ? 8 : 4; }

static ControlParams control_params(const gcsadmm_handle_s *h)
{
    const gcsadmm_params &p = h->params;
    return ControlParams{p.tau_incr, p.tau_decr, p.nu, p.eps_abs, p.eps_rel, h->plan.nx, h->plan.nmu, p.it_rho_limit, p.max_it};
}

// the inputs every vertex-step launch shares (step_args.h): the graph half (all the PROX solve reads: the rest stays zero) ...
static StepDesc make_step_graph(gcsadmm_handle h)
{
    StepDesc a{};
    a.inc_ptr = h->g.d_inc_ptr.get(); a.deg_in = h->g.d_deg_in.get(); a.inc_edge = h->g.d_inc_edge.get(); a.poly_ptr = h->g.d_poly_ptr.get();
    a.poly_A = h->g.d_poly_A.get(); a.poly_bc = h->g.d_poly_bc.get(); a.center = h->g.d_center.get();
    return a;
}
// ... and with the ADMM state, its column numbering, the loop's counters and the parameters of the run
static StepDesc make_step(gcsadmm_handle h, const gcsadmm_state *st)
{
    StepDesc a = make_step_graph(h);
    a.E = h->E; a.NI = h->NI; a.edge_major = h->edge_major;
    a.zedge = st->zedge; a.mu = st->mu; a.copy = st->copy; a.xv = st->xv; a.zv = st->zv; a.yv = st->yv;
    a.counters = h->loop.d_counters.get(); a.cb = h->loop.d_cb.get();
    a.eps_edge = h->params.eps_edge; a.ipm_tol = h->params.ipm_tol; a.ipm_max_iter = h->params.ipm_max_iter;
    a.warm = h->params.cold_start ? nullptr : h->g.d_warm.get(); a.warm_ptr = h->g.d_warm_ptr.get();
    return a;
}

// The generic vertices of a handle are split at create between the wavefront program (n = 2, degree <= 63: vertex_kernel.h)
// and the workgroup program (everything else, and all vertices of small graphs: vertex_wg.hip); the closed-form vertices
// ride in the trailing workgroups of whichever launch exists.
static WgLaunchDesc make_wg_desc(gcsadmm_handle h, const gcsadmm_state *st, bool with_special)
{
    WgLaunchDesc d;
    d.step = make_step(h, st);
    d.n = h->n; d.dtype = h->dtype; d.n_vtx = h->n_wg(); d.n_special = with_special ? h->n_special() : 0; d.lds_bytes = h->plan.wg_lds_bytes;
    d.vtx = h->g.d_wg_vtx.get(); d.special_vtx = h->g.d_special_vtx.get(); d.special_kind = h->g.d_special_kind.get(); d.box = h->plan.wg_box;
    d.order = h->g.d_wg_order.get(); d.unit_iters = h->g.d_wg_iters.get();
    return d;
}

static gcsadmm_k::TermLaunchDesc make_term_desc(gcsadmm_handle h, const gcsadmm_state *st)
{
    gcsadmm_k::TermLaunchDesc d;
    const CreatePlan &p = h->plan;
    d.step = make_step(h, st);
    d.n = h->n; d.dtype = h->dtype; d.count = p.n_term; d.threads = p.term_threads; d.lds_doubles = p.term_lds_doubles;
    for (int i = 0; i < 2; ++i) {
        d.t.vtx[i] = p.term_vtx[i]; d.t.is_src[i] = p.term_is_src[i]; d.t.ws_off[i] = p.term_ws_off[i]; d.t.rec_off[i] = p.term_rec_off[i];
    }
    d.t.ws = h->term.d_term_ws.get();
    d.t.rec = h->params.cold_start ? nullptr : h->term.d_term_rec.get();
    return d;
}

static VertexLaunchDesc make_launch_desc(gcsadmm_handle h, const gcsadmm_state *st)
{
    VertexLaunchDesc d;
    const CreatePlan &p = h->plan;
    d.step = make_step(h, st);
    d.n_waves = p.n_waves(); d.n_special = h->n_special(); d.all_m4 = p.all_m4; d.lds_bytes = p.lds_bytes; d.align_rows = p.align_rows;
    d.store_dl = p.store_dl; d.MM = p.wave_mm;
    d.wave_slot_ptr = h->g.d_wave_slot_ptr.get(); d.wave_vtx = h->g.d_wave_vtx.get(); d.special_vtx = h->g.d_special_vtx.get(); d.special_kind = h->g.d_special_kind.get();
    d.wave_order = h->g.d_wave_order.get(); d.wave_iters = h->g.d_wave_iters.get();
    return d;
}

// what a vertex-step launch is asked for; the default is the whole step alone
struct VertexLaunch {
    int part = -1;            // 0 / 1: the boundary / interior wavefronts of the overlapped partitioned loop (handles whose generic vertices
                              // are all on the wavefront program; the closed-form vertices ride with the boundary part)
    bool reorder = false;     // (a part) followed by the slowest-first reorder of the part's wavefronts
    const WgTailDesc *tail = nullptr;      // (gcsadmm_run on a handle that fuses, h->fuses()) the launch also runs the edge and control steps
};
static gcsadmm_status launch_vertex(gcsadmm_handle h, const gcsadmm_state *st, hipStream_t s, const VertexLaunch &req = {})
{
    const int part = req.part;
    const auto &g = h->g;
    const int n_waves = h->plan.n_waves();
    const gcsadmm_control_block *cb = h->loop.d_cb.get();
    auto launch_waves = [&](const VertexLaunchDesc &d) { with_state(h, [&](auto t) { launch_vertex_dim<2, decltype(t)>(d, s); }); };
    // terminals that are regions: their kernel runs on the auxiliary stream beside the launches below (it is a latency-bound solve in
    // one or two workgroups; the vertex launches do not wait for it, the caller's stream does at the end)
    const bool with_term = h->plan.n_term > 0 && part <= 0;
    if (with_term) {
        HIPCHK(h, hipEventRecord(h->term.ev_term_fork.get(), s));
        HIPCHK(h, hipStreamWaitEvent(h->term.term_stream.get(), h->term.ev_term_fork.get(), 0));
        gcsadmm_terminal_launch(make_term_desc(h, st), h->term.term_stream.get());
        HIPCHK(h, hipEventRecord(h->term.ev_term_join.get(), h->term.term_stream.get()));
    }
    struct Join {       // (every return path below joins)
        gcsadmm_handle h; hipStream_t s; bool on;
        ~Join() { if (on) (void)hipStreamWaitEvent(s, h->term.ev_term_join.get(), 0); }
    } join_{h, s, with_term};
    if (part >= 0) {
        const Overlap &o = h->overlap;
        VertexLaunchDesc d = make_launch_desc(h, st);
        const int off = part ? o.n_wave_b : 0, cnt = part ? n_waves - o.n_wave_b : o.n_wave_b;
        d.wave_order = o.d_split_order.get() + off;
        d.n_waves = cnt;
        if (part) d.n_special = 0;
        launch_waves(d);
        if (req.reorder && g.d_wave_iters)      // slowest first inside the part, on the part's own stream (its next launch reads the order)
            hipLaunchKernelGGL(reorder_kernel, dim3(1), dim3(REORDER_THREADS), 0, s, cnt, g.d_wave_iters.get(), o.d_split_order.get() + off, cb, o.d_split_ids.get() + off);
        HIPCHK(h, hipGetLastError());
        return GCSADMM_OK;
    }
    const bool special_on_wave = n_waves > 0;
    if (n_waves > 0) launch_waves(make_launch_desc(h, st));
    if (h->n_wg() > 0 || (!special_on_wave && h->n_special() > 0)) {
        WgLaunchDesc d = make_wg_desc(h, st, !special_on_wave);
        if (req.tail) d.tail = *req.tail;
        if (h->plan.wg_t512) gcsadmm_wg_launch_t512(d, s);
        else gcsadmm_wg_launch(d, s);
    }
    if (h->n_split() > 0) {      // the vertices too large for LDS: the split form, units in the handle's workspace
        WgLaunchDesc d = make_wg_desc(h, st, false);
        d.n_vtx = h->n_split(); d.vtx = g.d_split_vtx.get(); d.lds_bytes = h->plan.split_lds_bytes; d.order = nullptr; d.unit_iters = nullptr;
        gcsadmm_wg_launch_split(d, WgSplitArgs{g.d_split_ws.get(), g.d_split_off.get()}, s);
    }
    if (++h->vertex_steps % REORDER_EVERY == 0) {      // slowest-first dispatch of the following launches (graphs that need more than one round)
        if (g.d_wave_order) hipLaunchKernelGGL(reorder_kernel, dim3(1), dim3(REORDER_THREADS), 0, s, n_waves, g.d_wave_iters.get(), g.d_wave_order.get(), cb);
        if (g.d_wg_order) hipLaunchKernelGGL(reorder_kernel, dim3(1), dim3(REORDER_THREADS), 0, s, h->n_wg(), g.d_wg_iters.get(), g.d_wg_order.get(), cb);
    }
    HIPCHK(h, hipGetLastError());
    return GCSADMM_OK;
}

// the arguments of an edge-step launch (the kernarg of edge_kernel, or a member's entry of the batch table)
template <class T> static EdgeArgs<T> make_edge_args(gcsadmm_handle h, const gcsadmm_state *st)
{
    EdgeArgs<T> a;
    a.E = h->E; a.NI = h->NI; a.c = h->c;
    a.edge_inc_tail = h->edge_major ? nullptr : h->g.d_edge_inc_tail.get(); a.edge_inc_head = h->edge_major ? nullptr : h->g.d_edge_inc_head.get();
    a.inc_counted = h->g.d_inc_counted.get(); a.edge_counted = h->g.d_edge_counted.get();
    a.copy = (const T *)st->copy; a.zedge = (T *)st->zedge; a.mu = (T *)st->mu; a.partials = h->loop.d_partials.get();
    return a;
}

// the fused tail of the in-LDS launch (gcsadmm_run on handles that fuse): what launch_edge would hand edge_kernel MODE 1, beside make_wg_desc
static WgTailDesc make_wg_tail(gcsadmm_handle h, const gcsadmm_state *st, double *trace)
{
    WgTailDesc t;
    t.enabled = 1;
    t.edge = retype<void>(make_edge_args<char>(h, st));      // (untyped: the launch casts the three state pointers back)
    t.cb = h->loop.d_cb.get(); t.sums = h->loop.d_sums.get(); t.cp = control_params(h);
    t.counters = h->loop.d_counters.get(); t.trace = trace; t.ticket = h->loop.d_ticket.get();
    return t;
}

// How an edge step ends (the MODE of edge_kernel): the partials of every workgroup and a finalize launch (the separate steps of the
// ABI); with the control step in the same launch, run by the single workgroup or by the last one to finish (gcsadmm_run; the trace may
// be null); the six sums of a partition, reduced by the last workgroup (the partitioned loop)
enum class EdgeMode { Partials = 0, ControlOneGroup = 1, ControlLastGroup = 2, Sums6 = 3 };
static EdgeMode edge_mode_with_control(const gcsadmm_handle_s *h) { return h->plan.edge_blocks == 1 ? EdgeMode::ControlOneGroup : EdgeMode::ControlLastGroup; }

static gcsadmm_status launch_edge(gcsadmm_handle h, const gcsadmm_state *st, double *sums, hipStream_t s, EdgeMode mode, double *trace = nullptr)
{
    const ControlParams cp = control_params(h);
    const int edge_blocks = h->plan.edge_blocks;
    with_state(h, [&](auto t) {
        using T = decltype(t);
        const EdgeArgs<T> a = make_edge_args<T>(h, st);
        // one kernel instantiation per (state type, mode, words per copy c = 2n + 1, edges per thread)
        dispatch_dim<1, 2, 3, 4, 5, 6, 7, 8>(h->n, [&](auto N) {
            dispatch_dim<0, 1, 2, 3>((int)mode, [&](auto M) {
                constexpr int C = 2 * decltype(N)::value + 1;
                auto go = [&](auto U) {
                    hipLaunchKernelGGL((edge_kernel<T, decltype(M)::value, C, decltype(U)::value>), dim3(edge_blocks), dim3(EDGE_BLOCK), 0, s, a, h->loop.d_cb.get(), sums, cp,
                                       h->loop.d_counters.get(), trace, h->loop.d_ticket.get());
                };
                if (h->plan.edge_unroll > 1) go(std::integral_constant<int, edge_unroll<T, C>()>());
                else go(std::integral_constant<int, 1>());
            });
        });
        if (mode == EdgeMode::Partials) hipLaunchKernelGGL(finalize_kernel, dim3(1), dim3(256), 0, s, a.partials, edge_blocks, sums, h->loop.d_cb.get());
    });
    HIPCHK(h, hipGetLastError());
    return GCSADMM_OK;
}

static bool state_ok(gcsadmm_handle h, const gcsadmm_state *st)
{
    if (!h || !st || !st->copy || !st->mu || !st->zedge || !st->xv || !st->zv || !st->yv) { if (h) h->err = "null state pointer"; return false; }
    if (!h->params_set) { h->err = "gcsadmm_reset has not been called"; return false; }
    return true;
}

// ---- halo of a vertex partition: host-side helpers (C++ linkage); what the lists are refused for, the layout of the message and the
// split of the wavefronts are halo_plan.h's ----
// the three halo calls of the ABI: a state that can run, and a halo to move
static bool need_halo(gcsadmm_handle h, const gcsadmm_state *st)
{
    if (!state_ok(h, st)) return false;
    if (!h->halo.attached()) { h->err = "no halo attached"; return false; }
    return true;
}

// gcsadmm_check_halo, and the head of gcsadmm_attach_comm: on the host alone
static gcsadmm_status check_halo_of(gcsadmm_handle h, int rank, int world, const gcsadmm_halo_desc *hd)
{
    if (h->halo.attached()) { h->err = "a communicator is already attached"; return GCSADMM_ERR_BAD_ARG; }
    return check_halo(h->plan.col_owned, h->NI, rank, world, hd, h->err);
}

// The overlapped loop's split (overlap_split, from the send list validated at attach), its second stream and its two events.  Leaves
// n_wave_b = 0 when there is nothing to split.
static gcsadmm_status overlap_setup(gcsadmm_handle h)
{
    Overlap &o = h->overlap;
    o = {};
    const OverlapSplit split = overlap_split(h->plan, h->V, h->halo.send_cols, h->overlap_mode, h->n_wg(), h->n_split());
    if (split.n_wave_b == 0) return GCSADMM_OK;
    o.n_wave_b = split.n_wave_b;
    HIPCHK(h, o.d_split_ids.upload(split.ids.data(), split.ids.size()));
    HIPCHK(h, o.d_split_order.upload(split.ids.data(), split.ids.size()));
    if (!h->g.d_wave_iters) HIPCHK(h, h->g.d_wave_iters.upload(nullptr, (size_t)h->plan.n_waves()));
    HIPCHK(h, create_owned(o.comm_stream, hipStreamCreateWithFlags, hipStreamNonBlocking));
    HIPCHK(h, create_owned(o.ev_boundary, hipEventCreateWithFlags, hipEventDisableTiming));
    HIPCHK(h, create_owned(o.ev_halo, hipEventCreateWithFlags, hipEventDisableTiming));
    return GCSADMM_OK;
}

static gcsadmm_status halo_upload(gcsadmm_handle h, const gcsadmm_halo_desc *hd)
{
    Halo &H = h->halo;
    static_cast<HaloPlan &>(H) = make_halo_plan(h->c, hd);
    const size_t esz = state_bytes(h), c = (size_t)h->c;
    HIPCHK(h, H.d_send_cols.upload(hd->send_cols, (size_t)H.n_send));
    HIPCHK(h, H.d_recv_cols.upload(hd->recv_cols, (size_t)H.n_recv));
    HIPCHK(h, H.d_send_base.upload(H.base.data(), (size_t)H.n_send));
    HIPCHK(h, H.d_send_stride.upload(H.stride.data(), (size_t)H.n_send));
    HIPCHK(h, H.d_recv_base.upload(H.base.data(), (size_t)H.n_recv));        // same block layout on the receiving side
    HIPCHK(h, H.d_recv_stride.upload(H.stride.data(), (size_t)H.n_recv));
    HIPCHK(h, H.d_sendbuf.alloc(std::max<size_t>((size_t)H.n_send * c * esz, 16)));
    HIPCHK(h, H.d_recvbuf.alloc(std::max<size_t>((size_t)H.n_recv * c * esz, 16)));
    // [0..6): this partition's five norms + inner failures, written by the edge step; [6..12): their sum over the ranks.  (Out of
    // place: after the stop test has fired the edge step no longer writes, and an in-place all-reduce would multiply the stale
    // values by `world` with every further iteration that was enqueued.)
    HIPCHK(h, H.d_sums6.upload(nullptr, 12));
    return GCSADMM_OK;
}

template <class T> static gcsadmm_status halo_pack(gcsadmm_handle h, const gcsadmm_state *st, hipStream_t s)
{
    const Halo &H = h->halo;
    if (H.n_send == 0) return GCSADMM_OK;
    const int tot = h->c * H.n_send;
    hipLaunchKernelGGL((halo_pack_kernel<T>), dim3((tot + 255) / 256), dim3(256), 0, s, h->c, H.n_send, h->NI, H.d_send_cols.get(),
                       H.d_send_base.get(), H.d_send_stride.get(), (const T *)st->copy, (T *)H.d_sendbuf.get(), h->loop.d_cb.get());
    HIPCHK(h, hipGetLastError());
    return GCSADMM_OK;
}
template <class T> static gcsadmm_status halo_unpack(gcsadmm_handle h, const gcsadmm_state *st, hipStream_t s)
{
    const Halo &H = h->halo;
    if (H.n_recv == 0) return GCSADMM_OK;
    const int tot = h->c * H.n_recv;
    hipLaunchKernelGGL((halo_unpack_kernel<T>), dim3((tot + 255) / 256), dim3(256), 0, s, h->c, H.n_recv, h->NI, H.d_recv_cols.get(),
                       H.d_recv_base.get(), H.d_recv_stride.get(), (const T *)H.d_recvbuf.get(), (T *)st->copy, h->loop.d_cb.get());
    HIPCHK(h, hipGetLastError());
    return GCSADMM_OK;
}

// the grouped point-to-point exchange of the packed halo (one message per neighbour and direction)
static gcsadmm_status halo_transfer(gcsadmm_handle h, hipStream_t s)
{
    const Halo &H = h->halo;
    if (H.peers.empty()) return GCSADMM_OK;
    if (!h->comm) { h->err = "halo exchange needs a communicator (gcsadmm_attach_comm with an id)"; return GCSADMM_ERR_BAD_ARG; }
    const ncclDataType_t dt = h->dtype == GCSADMM_F64 ? ncclFloat64 : ncclFloat32;
    const size_t esz = state_bytes(h);
    NCCLCHK(h, rccl().GroupStart());
    for (size_t p = 0; p < H.peers.size(); ++p) {
        const size_t off = (size_t)H.peer_off[p] * h->c * esz, cnt = (size_t)H.peer_cnt[p] * h->c;
        NCCLCHK(h, rccl().Send(H.d_sendbuf.get() + off, cnt, dt, H.peers[p], (ncclComm_t)h->comm, s));
        NCCLCHK(h, rccl().Recv(H.d_recvbuf.get() + off, cnt, dt, H.peers[p], (ncclComm_t)h->comm, s));
    }
    NCCLCHK(h, rccl().GroupEnd());
    return GCSADMM_OK;
}

// pack, grouped send / recv, unpack: one halo exchange on one stream
static gcsadmm_status halo_exchange(gcsadmm_handle h, const gcsadmm_state *st, hipStream_t s)
{
    return with_state(h, [&](auto t) {
        using T = decltype(t);
        gcsadmm_status r;
        if ((r = halo_pack<T>(h, st, s)) != GCSADMM_OK) return r;
        if ((r = halo_transfer(h, s)) != GCSADMM_OK) return r;
        return halo_unpack<T>(h, st, s);
    });
}

// the timing entry points bracket their stages with events of the handle's pool: at least `count` of them
static gcsadmm_status ensure_events(gcsadmm_handle h, size_t count)
{
    while (h->events.size() < count) {
        Event e;
        HIPCHK(h, create_owned(e, hipEventCreateWithFlags, hipEventDefault));
        h->events.push_back(std::move(e));
    }
    return GCSADMM_OK;
}
// ... `stride` per iteration; *ms: the time from event `from` to event `to` of an iteration, summed over the k iterations
static gcsadmm_status elapsed_sum(gcsadmm_handle h, int stride, int k, int from, int to, float *ms)
{
    double acc = 0;
    for (int i = 0; i < k; ++i) {
        float t = 0;
        HIPCHK(h, hipEventElapsedTime(&t, h->events[stride * i + from].get(), h->events[stride * i + to].get()));
        acc += t;
    }
    *ms = (float)acc;
    return GCSADMM_OK;
}

// ---- batch of handles: host-side helpers (C++ linkage) ----
// the members as batch_plan.h sees them, and its verdict
static gcsadmm_status batch_plan_of(const std::vector<gcsadmm_handle> &members, unsigned flags, BatchPlan &bp, std::string &err)
{
    std::vector<BatchMember> m;
    for (gcsadmm_handle h : members)
        m.push_back(h ? BatchMember{h, &h->plan, h->n, h->dtype, h->device, h->n_wg(), h->n_special(), h->n_split(), h->halo.attached() || h->comm != nullptr}
                      : BatchMember{});
    return make_batch_plan(m.data(), (int)m.size(), bp, err, flags);
}

// the wave launches of a batch, one per group of its plan: `table` of group g follows those of the groups before it in d_wave_table
template <class F> static void each_wave_launch(const gcsadmm_batch_s *b, F &&f)
{
    const BatchPlan &bp = b->plan;
    size_t off = 0;
    for (const WaveGroup &g : bp.wave_groups) {
        f(WaveBatchLaunch{bp.dtype, g.all_m4, g.align_rows, g.store_dl, b->d_wave_table.get() + off, (unsigned)g.grid_x, (unsigned)g.members.size(), g.lds_bytes});
        off += wave_batch_entry_bytes(bp.dtype) * g.members.size();
    }
}

// the terminal launches of a batch, one per group of its plan, the tables laid out as the wave launches' are
template <class F> static void each_term_launch(const gcsadmm_batch_s *b, F &&f)
{
    const BatchPlan &bp = b->plan;
    size_t off = 0;
    for (const TermGroup &g : bp.term_groups) {
        f(gcsadmm_k::TermBatchLaunch{bp.n, bp.dtype, b->d_term_table.get() + off, (int)g.member.size(), g.threads, g.in_lds ? g.lds_doubles : 0});
        off += gcsadmm_terminal_batch_entry_bytes(bp.dtype) * g.member.size();
    }
}

// the members are released from the batch: it cannot run until it is bound again
static void batch_unbind(gcsadmm_batch_s *b)
{
    for (gcsadmm_handle h : b->members)
        if (h && h->batch == b) h->batch = nullptr;
    b->bound = false;
}

// a handle that is destroyed leaves the batches that list it: they keep a null member and refuse to be bound again
static void batches_forget(gcsadmm_handle h)
{
    for (gcsadmm_batch_s *b : h->batches) {
        batch_unbind(b);
        std::replace(b->members.begin(), b->members.end(), h, (gcsadmm_handle) nullptr);
    }
}

// gcsadmm_batch_create / _ex, host part: the arguments, the batch object and its plan; a refusal leaves its text in g_create_error
static gcsadmm_status batch_make(const gcsadmm_handle *members, int count, unsigned flags, gcsadmm_batch_s **out, std::unique_ptr<gcsadmm_batch_s> &b)
{
    auto fail = [&](gcsadmm_status st, const std::string &msg) { g_create_error = msg; return st; };
    if (!out) return fail(GCSADMM_ERR_BAD_ARG, "null output pointer");
    if (flags & ~(unsigned)(GCSADMM_BATCH_LARGE | GCSADMM_BATCH_TERMINALS)) return fail(GCSADMM_ERR_BAD_ARG, "unknown batch flag");
    if (!members || count < 1) return fail(GCSADMM_ERR_BAD_ARG, "a batch needs at least one member");
    b = std::make_unique<gcsadmm_batch_s>();
    b->members.assign(members, members + count);
    b->flags = flags;
    std::string msg;
    const gcsadmm_status st = batch_plan_of(b->members, flags, b->plan, msg);
    if (st != GCSADMM_OK) return fail(st, msg);
    b->device = b->plan.device;
    return GCSADMM_OK;
}

// ... device part, under the guard of the batch's device (`guard`: what taking it returned): the tables, the LDS limits of the kernels
// that need more than 48 KB; then the members list the batch and *out takes it
static gcsadmm_status batch_finish(std::unique_ptr<gcsadmm_batch_s> &b, hipError_t guard, gcsadmm_batch_s **out)
{
    const BatchPlan &plan = b->plan;
    const size_t count = (size_t)plan.count;
    size_t wave_entries = 0, term_entries = 0;
    for (const WaveGroup &g : plan.wave_groups) wave_entries += g.members.size();
    for (const TermGroup &g : plan.term_groups) term_entries += g.member.size();
    hipError_t e = guard;
    if (e == hipSuccess) e = b->d_vertex_table.alloc(gcsadmm_wg_batch_entry_bytes(plan.dtype) * std::max<size_t>(plan.wg_members.size(), 1));
    if (e == hipSuccess) e = b->d_edge_table.alloc((plan.dtype == GCSADMM_F64 ? sizeof(EdgeBatchEntry<double>) : sizeof(EdgeBatchEntry<float>)) * count);
    if (e == hipSuccess && wave_entries > 0) e = b->d_wave_table.alloc(wave_batch_entry_bytes(plan.dtype) * wave_entries);
    if (e == hipSuccess && term_entries > 0) e = b->d_term_table.alloc(gcsadmm_terminal_batch_entry_bytes(plan.dtype) * term_entries);
    if (e == hipSuccess && term_entries > 0) e = create_owned(b->term_stream, hipStreamCreateWithFlags, hipStreamNonBlocking);
    if (e == hipSuccess && term_entries > 0) e = create_owned(b->ev_term_fork, hipEventCreateWithFlags, hipEventDisableTiming);
    if (e == hipSuccess && term_entries > 0) e = create_owned(b->ev_term_join, hipEventCreateWithFlags, hipEventDisableTiming);
    if (e == hipSuccess) e = b->d_cbs.alloc(count);
    if (e == hipSuccess) e = b->d_poll.upload(nullptr, 2 * count);
    if (e == hipSuccess && plan.vertex_lds_bytes > 48 * 1024) e = gcsadmm_wg_set_batch_lds(plan.n, plan.dtype, plan.vertex_lds_bytes);
    each_wave_launch(b.get(), [&](const WaveBatchLaunch &w) {
        if (e == hipSuccess && w.lds_bytes > 48 * 1024) e = wave_batch_set_lds(w);
    });
    if (e != hipSuccess) {
        g_create_error = b->err = std::string("gcsadmm_batch_create: ") + hipGetErrorString(e);
        return GCSADMM_ERR_HIP;
    }
    b->poll_host.resize(2 * count);
    for (gcsadmm_handle h : b->members) h->batches.reserve(h->batches.size() + 1);      // (a push that failed half way would leave members listing a batch that is gone)
    for (gcsadmm_handle h : b->members) h->batches.push_back(b.get());
    *out = b.release();
    return GCSADMM_OK;
}

static gcsadmm_status need_bound(gcsadmm_batch_s *b)
{
    if (!b->bound) b->err = "gcsadmm_batch_bind has not been called";
    return bad_unless(b->bound);
}

// ---- state transfer (state_transfer_core.h): host-side helpers of the four export / import entry points ----
// the checks and the table of a call are the header's (transfer_add on a TransferHandle): what it reads of a handle.  The two arrays of
// edge ends are uploaded by the handle's first transfer (transfer_ends), so the entries take their pointers there
static TransferHandle transfer_handle(const gcsadmm_handle_s *h)
{
    return TransferHandle{h->n, h->dtype, h->V, h->E, h->NI, h->edge_major, h->plan.edges_ascending, h->params_set, h->g.d_edge_tail.get(), h->g.d_edge_head.get(),
                          h->g.d_edge_inc_tail.get(), h->g.d_edge_inc_head.get(), h->loop.d_cb.get()};
}

// one call: its table, and the handle of every entry
struct TransferJob {
    TransferCall call;
    std::vector<gcsadmm_handle> handles;
};
// under the guard, before the launch: the edge ends of every handle of the job are on the device and in its entry
template <class O> static gcsadmm_status transfer_ends(O *obj, TransferJob &job)
{
    for (size_t i = 0; i < job.handles.size(); ++i) {
        gcsadmm_handle h = job.handles[i];
        if (!h->g.d_edge_tail) HIPCHK(obj, h->g.d_edge_tail.upload(h->plan.edge_tail.data(), (size_t)h->E));
        if (!h->g.d_edge_head) HIPCHK(obj, h->g.d_edge_head.upload(h->plan.edge_head.data(), (size_t)h->E));
        job.call.table[i].edge_tail = h->g.d_edge_tail.get(); job.call.table[i].edge_head = h->g.d_edge_head.get();
    }
    return GCSADMM_OK;
}

// Upload the table and the ids into `buf` (the object's, kept from call to call), one launch for all members, then wait for it: the
// host arrays of `call` end with the call.  `obj`: the handle or batch whose err takes the text.
template <class O> static gcsadmm_status transfer_launch(O *obj, DevBuf<char> &buf, TransferJob &job, int dtype, bool exporting, hipStream_t s)
{
    TransferCall &call = job.call;
    if (call.table.empty()) return GCSADMM_OK;
    const gcsadmm_status ends = transfer_ends(obj, job);
    if (ends != GCSADMM_OK) return ends;
    const size_t table_bytes = sizeof(TransferEntry) * call.table.size(), id_bytes = sizeof(int32_t) * call.ids.size();
    HIPCHK(obj, buf.reserve(table_bytes + std::max<size_t>(id_bytes, 4)));
    const int32_t *d_ids = (const int32_t *)(buf.get() + table_bytes);
    for (size_t i = 0; i < call.table.size(); ++i) call.table[i].vertex_id = d_ids + call.ids_at[i];
    HIPCHK(obj, hipMemcpyAsync(buf.get(), call.table.data(), table_bytes, hipMemcpyHostToDevice, s));
    if (id_bytes) HIPCHK(obj, hipMemcpyAsync(buf.get() + table_bytes, call.ids.data(), id_bytes, hipMemcpyHostToDevice, s));
    const TransferEntry *table = (const TransferEntry *)buf.get();
    with_state_type(dtype == GCSADMM_F64, [&](auto t) {
        using T = decltype(t);
        if (exporting) hipLaunchKernelGGL((state_export_kernel<T>), dim3(call.blocks), dim3(TRANSFER_BLOCK), 0, s, table, (int)call.table.size());
        else hipLaunchKernelGGL((state_import_kernel<T>), dim3(call.blocks), dim3(TRANSFER_BLOCK), 0, s, table, (int)call.table.size());
    });
    HIPCHK(obj, hipGetLastError());
    HIPCHK(obj, hipStreamSynchronize(s));
    return GCSADMM_OK;
}

// the members of a batch call that have a snapshot, checked and entered; nothing is entered unless all pass
template <class S> static gcsadmm_status transfer_add_batch(gcsadmm_batch_s *b, TransferJob &job, const int32_t *const *vertex_ids, S *const *snapshots, bool exporting)
{
    if (need_bound(b) != GCSADMM_OK) return GCSADMM_ERR_BAD_ARG;
    if (!vertex_ids || !snapshots) { b->err = "null vertex_ids or snapshots"; return GCSADMM_ERR_BAD_ARG; }
    for (size_t i = 0; i < b->members.size(); ++i) {
        if (!snapshots[i]) continue;
        const gcsadmm_status st = transfer_add(job.call, transfer_handle(b->members[i]), &b->states[i], vertex_ids[i], snapshots[i], exporting, "member " + std::to_string(i) + ": ", b->err);
        if (st != GCSADMM_OK) return st;
        job.handles.push_back(b->members[i]);
    }
    return GCSADMM_OK;
}

// the one member of a solo call
static gcsadmm_status transfer_add_solo(TransferJob &job, gcsadmm_handle h, const gcsadmm_state *st, const int32_t *vertex_id, const gcsadmm_snapshot *snap, bool exporting)
{
    const gcsadmm_status r = transfer_add(job.call, transfer_handle(h), st, vertex_id, snap, exporting, "", h->err);
    if (r == GCSADMM_OK) job.handles.push_back(h);
    return r;
}

// what an export reports back: the sizes it wrote
static void transfer_exported(const gcsadmm_handle_s *h, gcsadmm_snapshot *snap) { snap->V = h->V; snap->E = h->E; }

// one vertex launch of the workgroup program over the members that have something in it, one of the wavefront program per group
// (GCSADMM_BATCH_LARGE alone has any) and one edge + control launch for the whole batch.  GCSADMM_BATCH_TERMINALS: the terminal launches,
// one per group, run on the batch's auxiliary stream beside the vertex launches -- forked before them, joined before the edge step, as
// launch_vertex does for a solo handle; no member's own terminal stream is used
static gcsadmm_status launch_batch_iteration(gcsadmm_batch_s *b, hipStream_t s)
{
    const BatchPlan &bp = b->plan;
    const bool with_term = !bp.term_groups.empty();
    if (with_term) {
        HIPCHK(b, hipEventRecord(b->ev_term_fork.get(), s));
        HIPCHK(b, hipStreamWaitEvent(b->term_stream.get(), b->ev_term_fork.get(), 0));
        each_term_launch(b, [&](const gcsadmm_k::TermBatchLaunch &t) { gcsadmm_terminal_launch_batch(t, b->term_stream.get()); });
        HIPCHK(b, hipEventRecord(b->ev_term_join.get(), b->term_stream.get()));
    }
    if (bp.vertex_grid_x > 0)
        gcsadmm_wg_launch_batch(WgBatchLaunch{bp.n, bp.dtype, bp.box, b->d_vertex_table.get(), (unsigned)bp.vertex_grid_x, (unsigned)bp.wg_members.size(), bp.vertex_lds_bytes}, s);
    each_wave_launch(b, [&](const WaveBatchLaunch &w) { wave_batch_launch(w, s); });
    if (with_term) HIPCHK(b, hipStreamWaitEvent(s, b->ev_term_join.get(), 0));
    with_state_type(bp.dtype == GCSADMM_F64, [&](auto t) {
        using T = decltype(t);
        const auto *table = (const EdgeBatchEntry<T> *)b->d_edge_table.get();
        dispatch_dim<1, 2, 3, 4, 5, 6, 7, 8>(bp.n, [&](auto N) {
            hipLaunchKernelGGL((edge_batch_kernel<T, 2 * decltype(N)::value + 1>), dim3(bp.edge_grid_x, bp.count), dim3(EDGE_BLOCK), 0, s, table);
        });
    });
    HIPCHK(b, hipGetLastError());
    return GCSADMM_OK;
}

// The end of an iteration of the partitioned loop, on the caller's stream: the edge step (sums + failure count, one launch), the
// all-reduce of the six doubles where a communicator is attached, the control step fed from the reduced sums.  ev != nullptr (the
// stage-timed serial schedule): three events, recorded after the edge step, after the all-reduce and after the control step.
static gcsadmm_status partitioned_tail(gcsadmm_handle h, const gcsadmm_state *st, double *trace_dev, hipStream_t s, const Event *ev)
{
    double *sums6 = h->halo.d_sums6.get();
    gcsadmm_status r = launch_edge(h, st, sums6, s, EdgeMode::Sums6);
    if (r != GCSADMM_OK) return r;
    if (ev) HIPCHK(h, hipEventRecord(ev[0].get(), s));
    const double *reduced = sums6;
    if (h->comm) {
        NCCLCHK(h, rccl().AllReduce(sums6, sums6 + 6, 6, ncclFloat64, ncclSum, (ncclComm_t)h->comm, s));
        reduced = sums6 + 6;
    }
    if (ev) HIPCHK(h, hipEventRecord(ev[1].get(), s));
    hipLaunchKernelGGL(control_kernel, dim3(1), dim3(1), 0, s, h->loop.d_cb.get(), reduced, control_params(h), h->loop.d_counters.get(), trace_dev, true);
    HIPCHK(h, hipGetLastError());
    if (ev) HIPCHK(h, hipEventRecord(ev[2].get(), s));
    return GCSADMM_OK;
}

// =================================================================================================
// vertex partitions across GPUs: one handle per rank, RCCL over xGMI.
// Per iteration, all on one stream with no host synchronisation:
//   vertex step -> pack the cut edges' copies per neighbour -> grouped ncclSend / ncclRecv -> unpack into the ghost columns
//   -> edge step on local + ghost columns -> ncclAllReduce(sum) of the five norms and the inner-failure count (6 doubles)
//   -> control (every rank takes the same decision from the same numbers).
// Both messages are latency-bound at every configuration of BASELINE.json (about 25 KB per boundary of the 100k lattice,
// 48 bytes for the all-reduce).
// =================================================================================================
// one loop for gcsadmm_run_partitioned and its event-bracketed twin: ev != nullptr records 6 events per iteration on the stream
// (before / after the vertex step, after the halo exchange, after the edge step, after the all-reduce, after the control step)
static gcsadmm_status run_partitioned_loop(gcsadmm_handle h, const gcsadmm_state *st, int k, double *trace_dev, hipStream_t s, const Event *ev)
{
    if (!h->comm && h->world > 1) { h->err = "gcsadmm_run_partitioned needs a communicator (gcsadmm_attach_comm with an id)"; return GCSADMM_ERR_BAD_ARG; }
    gcsadmm_status r;
    // OVERLAPPED form (not for the stage-timed twin, whose events want one stream): the wavefronts that hold a vertex with a
    // cut edge are launched FIRST and on a second stream, with pack, grouped send / recv and unpack of the halo behind them; the interior
    // wavefronts are launched on the caller's stream at the same time, and the edge step waits for both.  Same kernels, same numbers: the
    // split only changes what runs when.
    //   s : [ev_boundary = previous iteration done] -> interior launch -> wait [ev_halo] -> edge step -> all-reduce -> control
    //   sc: wait [ev_boundary] -> boundary launch (+ closed-form vertices) -> pack -> send / recv -> unpack -> [ev_halo]
    // (The two launches must be CONCURRENT: one after the other on one stream each waits for its own slowest wavefront -- measured on a
    // strip of 12.6 k vertices, 348 -> 509 us per iteration.  RCCL orders the operations of one communicator across streams itself;
    // every rank issues them in the same order.)
    const Overlap &o = h->overlap;
    if (!ev && o.n_wave_b > 0 && h->overlap_mode != 2) {
        hipStream_t sc = o.comm_stream.get();
        for (int i = 0; i < k; ++i) {
            const bool reorder = ++h->vertex_steps % REORDER_EVERY == 0;
            HIPCHK(h, hipEventRecord(o.ev_boundary.get(), s));
            HIPCHK(h, hipStreamWaitEvent(sc, o.ev_boundary.get(), 0));
            if ((r = launch_vertex(h, st, sc, VertexLaunch{0, reorder})) != GCSADMM_OK) return r;
            if ((r = halo_exchange(h, st, sc)) != GCSADMM_OK) return r;
            HIPCHK(h, hipEventRecord(o.ev_halo.get(), sc));
            if ((r = launch_vertex(h, st, s, VertexLaunch{1, reorder})) != GCSADMM_OK) return r;
            HIPCHK(h, hipStreamWaitEvent(s, o.ev_halo.get(), 0));
            if ((r = partitioned_tail(h, st, trace_dev, s, nullptr)) != GCSADMM_OK) return r;
        }
        // the caller's stream is the one the caller synchronises: nothing of this call may still run on the other
        HIPCHK(h, hipEventRecord(o.ev_halo.get(), sc));
        HIPCHK(h, hipStreamWaitEvent(s, o.ev_halo.get(), 0));
        return GCSADMM_OK;
    }
    for (int i = 0; i < k; ++i) {
        if (ev) HIPCHK(h, hipEventRecord(ev[6 * i + 0].get(), s));
        if ((r = launch_vertex(h, st, s)) != GCSADMM_OK) return r;
        if (ev) HIPCHK(h, hipEventRecord(ev[6 * i + 1].get(), s));
        if ((r = halo_exchange(h, st, s)) != GCSADMM_OK) return r;
        if (ev) HIPCHK(h, hipEventRecord(ev[6 * i + 2].get(), s));
        if ((r = partitioned_tail(h, st, trace_dev, s, ev ? ev + 6 * i + 3 : nullptr)) != GCSADMM_OK) return r;
    }
    return GCSADMM_OK;
}
// what both entry points of that loop refuse
static gcsadmm_status need_partitioned(gcsadmm_handle h, bool args_ok)
{
    if (!args_ok) return GCSADMM_ERR_BAD_ARG;
    if (!h->halo.attached()) h->err = "gcsadmm_attach_comm has not been called";
    return bad_unless(h->halo.attached());
}

// gcsadmm_batch_create with flags (include/gcsadmm.h).  It stands HERE, before the block of entry points, and carries its linkage itself:
// tests/test_build.py reads every function of that block by its first parameter, a handle or a batch, and has a closed list of the
// creates, which have neither; this create takes the array of handles, so the block's rules have no case for it.  What they are there
// for holds: nothing touches the device before the guard, which is guarded_entry's, taken on the batch that batch_make has just made.
// (gcsadmm_batch_create does the same job with a DeviceGuard of its own, because the same test wants that guard written in its body and
// in no function but the listed creates and guarded_entry: two shapes around the shared batch_make / batch_finish, not one.)
extern "C" gcsadmm_status gcsadmm_batch_create_ex(const gcsadmm_handle *members, int32_t count, int32_t flags, struct gcsadmm_batch_s **out)
{
    if (out) *out = nullptr;
    return entry(g_create_error, [&]() -> gcsadmm_status {
        std::unique_ptr<gcsadmm_batch_s> b;
        gcsadmm_status st = batch_make(members, count, (unsigned)flags, out, b);
        if (st != GCSADMM_OK) return st;
        st = guarded_entry(b.get(), [] { return GCSADMM_OK; }, [&] { return batch_finish(b, hipSuccess, out); });
        if (b) g_create_error = b->err;      // (the guard's own failure: the text is the batch's, and the batch goes)
        return st;
    });
}

// Every entry point that takes a handle or a batch is one handle_entry / batch_entry (the argument checks, then the work under the
// object's device), and none calls another: the loops and the shared checks are the helpers above.  Plain -- they never reach the
// device -- are the two last_error calls, the two queries, set_fused_tail, halo_buffers and check_halo.
extern "C" {

const char *gcsadmm_last_error(gcsadmm_handle h) { return h ? h->err.c_str() : g_create_error.c_str(); }

void gcsadmm_destroy(gcsadmm_handle h)
{
    if (!h) return;
    DeviceGuard device_guard_(h->device);      // the owners release on the handle's device
    batches_forget(h);
    if (h->comm && rccl().ok()) (void)rccl().CommDestroy((ncclComm_t)h->comm);
    delete h;
}

gcsadmm_status gcsadmm_create(const gcsadmm_graph_desc *g, gcsadmm_handle *out)
{
    if (out) *out = nullptr;
    return entry(g_create_error, [&]() -> gcsadmm_status {
        auto fail = [&](gcsadmm_status st, const std::string &msg) { g_create_error = msg; return st; };
        std::string msg;
        gcsadmm_status st;
        if (!out) return fail(GCSADMM_ERR_BAD_ARG, "null descriptor or output pointer");
        if ((st = check_graph_desc(g, msg)) != GCSADMM_OK) return fail(st, msg);
        int ndev = 0;
        if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) return fail(GCSADMM_ERR_NO_DEVICE, "no HIP device");
        if (g->device < 0 || g->device >= ndev) return fail(GCSADMM_ERR_BAD_ARG, "device ordinal out of range");
        CreatePlan plan;
        if ((st = make_create_plan(*g, plan, msg)) != GCSADMM_OK) return fail(st, msg);

        const int V = g->num_vertices, E = g->num_edges, n = g->n, NIo = g->inc_ptr[V], MT = g->poly_ptr[V];
        DeviceGuard device_guard_(g->device);      // (declared before the handle: whatever has been filled is released under the guard)
        auto h = std::make_unique<gcsadmm_handle_s>();
        h->n = n; h->V = V; h->E = E; h->NI = g->num_incidences; h->c = 2 * n + 1;
        h->edge_major = g->edge_major_columns; h->src = g->src; h->dst = g->dst;
        h->dtype = g->state_dtype; h->device = g->device;
        h->plan = std::move(plan);
        CreatePlan &p = h->plan;
        auto bail = [&](hipError_t e, const char *what) { return fail(GCSADMM_ERR_HIP, std::string(what) + ": " + hipGetErrorString(e)); };
        hipError_t e;
        if ((e = device_guard_.err) != hipSuccess) return bail(e, "hipSetDevice");
#define UP(group, dst, src, cnt) if ((e = h->group.dst.upload(src, (size_t)(cnt))) != hipSuccess) return bail(e, "upload " #dst)
        UP(g, d_inc_ptr, g->inc_ptr, V + 1);
        UP(g, d_deg_in, p.deg_in.data(), V);
        UP(g, d_inc_edge, g->inc_edge, NIo);
        UP(g, d_poly_ptr, g->poly_ptr, V + 1);
        UP(g, d_edge_inc_tail, g->edge_inc_tail, E);
        UP(g, d_edge_inc_head, g->edge_inc_head, E);
        UP(g, d_wave_slot_ptr, p.wave_slot_ptr.data(), p.wave_slot_ptr.size());
        UP(g, d_wave_vtx, p.wave_vtx.data(), p.wave_vtx.size());
        UP(g, d_special_vtx, p.special_vtx.data(), p.special_vtx.size());
        UP(g, d_special_kind, p.special_kind.data(), p.special_kind.size());
        UP(g, d_wg_vtx, p.wg_vtx.data(), p.wg_vtx.size());
        if (!p.split_vtx.empty()) {
            UP(g, d_split_vtx, p.split_vtx.data(), p.split_vtx.size());
            UP(g, d_split_off, p.split_off.data(), p.split_off.size());
            UP(g, d_split_ws, nullptr, p.split_doubles);
        }
        UP(g, d_poly_A, g->poly_A, (size_t)MT * n);
        UP(g, d_poly_bc, p.bc.data(), MT);
        UP(g, d_center, g->center, (size_t)V * n);
        if (g->inc_counted) UP(g, d_inc_counted, g->inc_counted, g->num_incidences);
        if (g->edge_counted) UP(g, d_edge_counted, g->edge_counted, E);
        UP(loop, d_cb, nullptr, 1);
        UP(loop, d_counters, nullptr, 2);
        UP(loop, d_partials, nullptr, (size_t)p.edge_blocks * 5);
        UP(loop, d_sums, nullptr, 5);
        UP(loop, d_ticket, nullptr, 1);
        if (p.n_term > 0) {       // region terminals: workspace, an auxiliary stream and the fork / join events
            UP(term, d_term_ws, nullptr, p.term_ws_doubles);
            UP(term, d_term_rec, nullptr, p.term_rec_doubles);
            if ((e = create_owned(h->term.term_stream, hipStreamCreateWithFlags, hipStreamNonBlocking)) != hipSuccess) return bail(e, "hipStreamCreate");
            if ((e = create_owned(h->term.ev_term_fork, hipEventCreateWithFlags, hipEventDisableTiming)) != hipSuccess) return bail(e, "hipEventCreate");
            if ((e = create_owned(h->term.ev_term_join, hipEventCreateWithFlags, hipEventDisableTiming)) != hipSuccess) return bail(e, "hipEventCreate");
        }
        UP(g, d_warm_ptr, p.warm_ptr.data(), V + 1);
        UP(g, d_warm, nullptr, p.warm_ptr[V]);
        // slowest-first dispatch: only where a launch needs more than one round of the chip (small graphs run all at once)
        const int n_waves = p.n_waves(), n_wg = h->n_wg();
        h->iota.resize(std::max(std::max(n_waves, n_wg), 1));
        for (size_t i = 0; i < h->iota.size(); ++i) h->iota[i] = (int)i;
        if (p.wave_reorder) { UP(g, d_wave_iters, nullptr, n_waves); UP(g, d_wave_order, h->iota.data(), n_waves); }
        if (p.wg_reorder) { UP(g, d_wg_iters, nullptr, n_wg); UP(g, d_wg_order, h->iota.data(), n_wg); }
        UP(prox, d_prox_vtx, p.prox_vtx.data(), p.prox_vtx.size());
        UP(prox, d_prox_counters, nullptr, 2);
#undef UP
        // the plan's arrays that only fed an upload (the three the halo checks and the overlap split read stay: wave_slot_ptr, wave_vtx,
        // col_owned / col_vertex)
        auto release = [](auto &v) { v.clear(); v.shrink_to_fit(); };
        release(p.bc); release(p.deg_in); release(p.warm_ptr); release(p.prox_vtx); release(p.special_vtx); release(p.special_kind);
        release(p.wg_vtx); release(p.split_vtx); release(p.split_off);
        if (p.lds_bytes > 48 * 1024) {
            e = with_state(h.get(), [&](auto t) { return set_lds_attr<2, decltype(t)>(p.all_m4, p.lds_bytes); });
            if (e != hipSuccess) return bail(e, "hipFuncSetAttribute(MaxDynamicSharedMemorySize)");
        }
        if (p.wg_lds_bytes > 48 * 1024 && (e = p.wg_t512 ? gcsadmm_wg_set_lds_t512(h->n, h->dtype, p.wg_lds_bytes)
                                                          : gcsadmm_wg_set_lds(h->n, h->dtype, p.wg_lds_bytes)) != hipSuccess)
            return bail(e, "hipFuncSetAttribute(MaxDynamicSharedMemorySize, workgroup program)");
        if (p.split_lds_bytes > 48 * 1024 && (e = gcsadmm_wg_set_split_lds(h->n, h->dtype, p.split_lds_bytes)) != hipSuccess)
            return bail(e, "hipFuncSetAttribute(MaxDynamicSharedMemorySize, split workgroup program)");
        *out = h.release();
        return GCSADMM_OK;
    });
}

gcsadmm_status gcsadmm_reset(gcsadmm_handle h, const gcsadmm_params *p, void *stream)
{
    return handle_entry(h, [&] {
        if (!p) return GCSADMM_ERR_BAD_ARG;
        if (!(p->rho > 0) || p->max_it < 1 || !(p->ipm_tol > 0) || p->ipm_max_iter < 1) { h->err = "bad parameter"; return GCSADMM_ERR_BAD_ARG; }
        h->params = *p; h->params_set = true; ++h->resets;
        return GCSADMM_OK;
    }, [&] {
        gcsadmm_control_block cb{};
        cb.rho = p->rho; cb.mu_scale = 1.0; cb.it = 1; cb.status = GCSADMM_RUNNING;
        hipStream_t s = (hipStream_t)stream;
        HIPCHK(h, hipMemcpyAsync(h->loop.d_cb.get(), &cb, sizeof(cb), hipMemcpyHostToDevice, s));
        HIPCHK(h, h->loop.d_counters.zero(s));
        // a new run starts without warm-start records (runs from the same state are then identical, whatever ran before)
        HIPCHK(h, h->g.d_warm.zero(s));
        HIPCHK(h, h->term.d_term_rec.zero(s));
        h->vertex_steps = 0;
        const Overlap &o = h->overlap;
        if (o.d_split_order) HIPCHK(h, hipMemcpyAsync(o.d_split_order.get(), o.d_split_ids.get(), sizeof(int) * o.d_split_order.size(), hipMemcpyDeviceToDevice, s));
        for (const DevBuf<int> *order : {&h->g.d_wave_order, &h->g.d_wg_order})      // (h->iota outlives the copies)
            if (*order) HIPCHK(h, hipMemcpyAsync(order->get(), h->iota.data(), sizeof(int) * order->size(), hipMemcpyHostToDevice, s));
        HIPCHK(h, hipStreamSynchronize(s));   // cb is a stack object
        return GCSADMM_OK;
    });
}

gcsadmm_status gcsadmm_vertex_step(gcsadmm_handle h, const gcsadmm_state *st, void *stream)
{
    return handle_entry(h, [&] { return bad_unless(state_ok(h, st)); }, [&] { return launch_vertex(h, st, (hipStream_t)stream); });
}

gcsadmm_status gcsadmm_edge_step(gcsadmm_handle h, const gcsadmm_state *st, double *sums_dev, void *stream)
{
    return handle_entry(h, [&] { return bad_unless(state_ok(h, st) && sums_dev); },
                        [&] { return launch_edge(h, st, sums_dev, (hipStream_t)stream, EdgeMode::Partials); });
}

gcsadmm_status gcsadmm_control(gcsadmm_handle h, const double *sums_dev, double *trace_dev, void *stream)
{
    return handle_entry(h, [&] { return bad_unless(sums_dev && h->params_set); }, [&] {
        hipLaunchKernelGGL(control_kernel, dim3(1), dim3(1), 0, (hipStream_t)stream, h->loop.d_cb.get(), sums_dev, control_params(h), h->loop.d_counters.get(), trace_dev, false);
        HIPCHK(h, hipGetLastError());
        return GCSADMM_OK;
    });
}

gcsadmm_status gcsadmm_run(gcsadmm_handle h, const gcsadmm_state *st, int32_t k, double *trace_dev, void *stream)
{
    return handle_entry(h, [&] { return bad_unless(state_ok(h, st) && k >= 0); }, [&] {
        hipStream_t s = (hipStream_t)stream;
        gcsadmm_status r = GCSADMM_OK;
        if (h->fuses()) {      // small graphs: the last vertex workgroup runs the edge and control steps, one launch per iteration
            const WgTailDesc tail = make_wg_tail(h, st, trace_dev);
            for (int i = 0; i < k && r == GCSADMM_OK; ++i) r = launch_vertex(h, st, s, VertexLaunch{-1, false, &tail});
            return r;
        }
        const EdgeMode mode = edge_mode_with_control(h);      // edge step and control step in one launch
        for (int i = 0; i < k && r == GCSADMM_OK; ++i)
            if ((r = launch_vertex(h, st, s)) == GCSADMM_OK) r = launch_edge(h, st, h->loop.d_sums.get(), s, mode, trace_dev);
        return r;
    });
}

gcsadmm_status gcsadmm_comm_unique_id(void *id128)
{
    return entry(g_create_error, [&] {
        if (!id128) return GCSADMM_ERR_BAD_ARG;
        if (!rccl().ok()) { g_create_error = rccl().err; return GCSADMM_ERR_HIP; }
        static_assert(sizeof(ncclUniqueId) == 128, "ncclUniqueId is 128 bytes");
        ncclUniqueId id;
        if (rccl().GetUniqueId(&id) != ncclSuccess) { g_create_error = "ncclGetUniqueId failed"; return GCSADMM_ERR_HIP; }
        std::memcpy(id128, &id, sizeof(id));
        return GCSADMM_OK;
    });
}

gcsadmm_status gcsadmm_check_halo(gcsadmm_handle h, int32_t rank, int32_t world, const gcsadmm_halo_desc *halo)
{
    return h ? check_halo_of(h, rank, world, halo) : GCSADMM_ERR_BAD_ARG;
}

gcsadmm_status gcsadmm_attach_comm(gcsadmm_handle h, int32_t rank, int32_t world, const void *id128, const gcsadmm_halo_desc *halo)
{
    // everything that can fail on this rank alone comes first: a rank must not return an error while its peers wait in the collective
    return handle_entry(h, [&] {
        const gcsadmm_status st = check_halo_of(h, rank, world, halo);
        if (st != GCSADMM_OK) return st;
        if (id128 && !rccl().ok()) { h->err = rccl().err; return GCSADMM_ERR_HIP; }
        return GCSADMM_OK;
    }, [&] {
        h->rank = rank; h->world = world;
        const gcsadmm_status st = halo_upload(h, halo);
        if (st != GCSADMM_OK) { h->halo = {}; return st; }
        if (id128) {      // id128 == NULL: no communicator (the host moves the packed buffers itself; gcsadmm_run_partitioned needs one)
            ncclUniqueId id;
            std::memcpy(&id, id128, sizeof(id));
            ncclComm_t comm = nullptr;
            const ncclResult_t r = rccl().CommInitRank(&comm, world, id, rank);
            if (r != ncclSuccess) {      // not attached: the handle can be attached again
                h->err = std::string("ncclCommInitRank: ") + rccl().text(r);
                h->halo = {};
                return GCSADMM_ERR_HIP;
            }
            h->comm = comm;
        }
        return overlap_setup(h);
    });
}

gcsadmm_status gcsadmm_halo_pack(gcsadmm_handle h, const gcsadmm_state *st, void *stream)
{
    return handle_entry(h, [&] { return bad_unless(need_halo(h, st)); },
                        [&] { return with_state(h, [&](auto t) { return halo_pack<decltype(t)>(h, st, (hipStream_t)stream); }); });
}
gcsadmm_status gcsadmm_halo_unpack(gcsadmm_handle h, const gcsadmm_state *st, void *stream)
{
    return handle_entry(h, [&] { return bad_unless(need_halo(h, st)); },
                        [&] { return with_state(h, [&](auto t) { return halo_unpack<decltype(t)>(h, st, (hipStream_t)stream); }); });
}
gcsadmm_status gcsadmm_halo_buffers(gcsadmm_handle h, void **send_buf, void **recv_buf, int64_t *num_elements)
{
    if (!h || !h->halo.attached()) { if (h) h->err = "no halo attached"; return GCSADMM_ERR_BAD_ARG; }
    if (send_buf) *send_buf = h->halo.d_sendbuf.get();
    if (recv_buf) *recv_buf = h->halo.d_recvbuf.get();
    if (num_elements) *num_elements = (int64_t)h->c * h->halo.n_send;
    return GCSADMM_OK;
}

gcsadmm_status gcsadmm_halo_exchange(gcsadmm_handle h, const gcsadmm_state *st, void *stream)
{
    return handle_entry(h, [&] { return bad_unless(need_halo(h, st)); }, [&] { return halo_exchange(h, st, (hipStream_t)stream); });
}

gcsadmm_status gcsadmm_run_partitioned(gcsadmm_handle h, const gcsadmm_state *st, int32_t k, double *trace_dev, void *stream)
{
    return handle_entry(h, [&] { return need_partitioned(h, state_ok(h, st) && k >= 0); },
                        [&] { return run_partitioned_loop(h, st, k, trace_dev, (hipStream_t)stream, nullptr); });
}

gcsadmm_status gcsadmm_run_partitioned_timed(gcsadmm_handle h, const gcsadmm_state *st, int32_t k, double *trace_dev, void *stream,
                                             float *vertex_ms, float *halo_ms, float *edge_ms, float *reduce_ms)
{
    return handle_entry(h, [&] { return need_partitioned(h, state_ok(h, st) && k >= 0 && vertex_ms && halo_ms && edge_ms && reduce_ms); }, [&] {
        hipStream_t s = (hipStream_t)stream;
        gcsadmm_status r = ensure_events(h, (size_t)6 * k);
        if (r == GCSADMM_OK) r = run_partitioned_loop(h, st, k, trace_dev, s, h->events.data());
        if (r != GCSADMM_OK) return r;
        HIPCHK(h, hipStreamSynchronize(s));
        float *const out[4] = {vertex_ms, halo_ms, edge_ms, reduce_ms};
        const int from[4] = {0, 1, 2, 3}, to[4] = {1, 2, 3, 5};
        for (int q = 0; q < 4 && r == GCSADMM_OK; ++q) r = elapsed_sum(h, 6, k, from[q], to[q], out[q]);
        return r;
    });
}

int32_t gcsadmm_set_fused_tail(gcsadmm_handle h, int32_t mode)
{
    if (!h) return 0;
    h->fused_tail_mode = mode != 0;
    return h->fuses() ? 1 : 0;
}

gcsadmm_status gcsadmm_set_overlap(gcsadmm_handle h, int32_t mode, int32_t *boundary_units)
{
    return handle_entry(h, [&] {
        if (mode < 0 || mode > 2) return GCSADMM_ERR_BAD_ARG;
        if (boundary_units) *boundary_units = 0;
        return need_partitioned(h, true);
    }, [&] {
        h->overlap_mode = mode;
        const gcsadmm_status r = overlap_setup(h);
        if (boundary_units) *boundary_units = h->overlap.n_wave_b;
        return r;
    });
}

gcsadmm_status gcsadmm_comm_count(gcsadmm_handle h, int32_t *count)
{
    return handle_entry(h, [&] {
        if (!count) return GCSADMM_ERR_BAD_ARG;
        *count = 0;        // (stays 0 without a communicator: a single handle, or a host-side transport)
        if (h->comm && !rccl().CommCount) { h->err = "librccl lacks ncclCommCount"; return GCSADMM_ERR_HIP; }
        return GCSADMM_OK;
    }, [&] {
        int n = 0;
        if (h->comm) NCCLCHK(h, rccl().CommCount((ncclComm_t)h->comm, &n));
        *count = n;
        return GCSADMM_OK;
    });
}

gcsadmm_status gcsadmm_vertex_prox(gcsadmm_handle h, const double *q_dev, const double *c_dev, double *xv_dev, double *zv_dev,
                                   double *yv_dev, double ipm_tol, int32_t ipm_max_iter, int32_t *failures_host, void *stream)
{
    return handle_entry(h, [&] {
        if (!q_dev || !c_dev || !xv_dev || !zv_dev || !yv_dev || !(ipm_tol > 0) || ipm_max_iter < 1) { h->err = "bad prox argument"; return GCSADMM_ERR_BAD_ARG; }
        if (h->plan.prox_lds_bytes > 160 * 1024) { h->err = "facet count too large for LDS"; return GCSADMM_ERR_UNSUPPORTED; }
        if (h->plan.n_term > 0) { h->err = "the prox kernel (v1 x-update) takes its terminals as points; this graph has a terminal that is a region"; return GCSADMM_ERR_UNSUPPORTED; }
        return GCSADMM_OK;
    }, [&] {
        hipStream_t s = (hipStream_t)stream;
        HIPCHK(h, h->prox.d_prox_counters.zero(s));
        WgLaunchDesc d{};
        d.n = h->n; d.dtype = GCSADMM_F64; d.n_vtx = (int)h->prox.d_prox_vtx.size(); d.lds_bytes = h->plan.prox_lds_bytes; d.vtx = h->prox.d_prox_vtx.get();
        StepDesc &p = d.step = make_step_graph(h);     // the ADMM state, the edge tolerance and the warm start stay unset: the PROX solve reads none of them
        p.xv = xv_dev; p.zv = zv_dev; p.yv = yv_dev; p.counters = h->prox.d_prox_counters.get(); p.ipm_tol = ipm_tol; p.ipm_max_iter = ipm_max_iter;
        gcsadmm_wg_launch_prox(d, q_dev, c_dev, h->src, h->dst, s);
        HIPCHK(h, hipGetLastError());
        if (failures_host) {      // optional: synchronises the stream
            int cnt[2] = {0, 0};
            HIPCHK(h, hipMemcpyAsync(cnt, h->prox.d_prox_counters.get(), sizeof(cnt), hipMemcpyDeviceToHost, s));
            HIPCHK(h, hipStreamSynchronize(s));
            *failures_host = cnt[0];
        }
        return GCSADMM_OK;
    });
}

gcsadmm_status gcsadmm_run_timed(gcsadmm_handle h, const gcsadmm_state *st, int32_t k, double *trace_dev, void *stream,
                                 float *vertex_ms, int32_t *vertex_launches, float *edge_ms, int32_t *edge_launches)
{
    return handle_entry(h, [&] { return bad_unless(state_ok(h, st) && k >= 0 && vertex_ms && edge_ms && vertex_launches && edge_launches); }, [&] {
        hipStream_t s = (hipStream_t)stream;
        gcsadmm_status r = ensure_events(h, (size_t)4 * k);
        if (r != GCSADMM_OK) return r;
        const std::vector<Event> &ev = h->events;
        const EdgeMode mode = edge_mode_with_control(h);
        for (int i = 0; i < k; ++i) {
            HIPCHK(h, hipEventRecord(ev[4 * i + 0].get(), s));
            if ((r = launch_vertex(h, st, s)) != GCSADMM_OK) return r;
            HIPCHK(h, hipEventRecord(ev[4 * i + 1].get(), s));
            HIPCHK(h, hipEventRecord(ev[4 * i + 2].get(), s));
            if ((r = launch_edge(h, st, h->loop.d_sums.get(), s, mode, trace_dev)) != GCSADMM_OK) return r;
            HIPCHK(h, hipEventRecord(ev[4 * i + 3].get(), s));
        }
        HIPCHK(h, hipStreamSynchronize(s));
        if ((r = elapsed_sum(h, 4, k, 0, 1, vertex_ms)) != GCSADMM_OK || (r = elapsed_sum(h, 4, k, 2, 3, edge_ms)) != GCSADMM_OK) return r;
        *vertex_launches = k; *edge_launches = k;
        return GCSADMM_OK;
    });
}

gcsadmm_status gcsadmm_read_control(gcsadmm_handle h, gcsadmm_control_block *out, void *stream)
{
    return handle_entry(h, [&] { return bad_unless(out); }, [&] {
        HIPCHK(h, hipMemcpyAsync(out, h->loop.d_cb.get(), sizeof(*out), hipMemcpyDeviceToHost, (hipStream_t)stream));
        HIPCHK(h, hipStreamSynchronize((hipStream_t)stream));
        return GCSADMM_OK;
    });
}

gcsadmm_status gcsadmm_cost(gcsadmm_handle h, const gcsadmm_state *st, double eps_edge, double *cost_dev, void *stream)
{
    return handle_entry(h, [&] { return bad_unless(st && st->zv && st->zedge && cost_dev); }, [&] {
        with_state(h, [&](auto t) {
            using T = decltype(t);
            hipLaunchKernelGGL((cost_kernel<T>), dim3(1), dim3(256), 0, (hipStream_t)stream, h->V, h->E, h->n, st->zv,
                               (const T *)st->zedge, h->g.d_edge_counted.get(), eps_edge, cost_dev);
        });
        HIPCHK(h, hipGetLastError());
        return GCSADMM_OK;
    });
}

#ifdef GCS_PHASE_TIMING
int gcsadmm_debug_sub_cycles(unsigned long long *out16)
{
    return (int)hipMemcpyFromSymbol(out16, HIP_SYMBOL(g_sub_cycles), 16 * sizeof(unsigned long long));
}

int gcsadmm_debug_phase_cycles(unsigned long long *out64)
{
    return (int)hipMemcpyFromSymbol(out64, HIP_SYMBOL(g_phase_cycles), 64 * sizeof(unsigned long long));
}
#endif

gcsadmm_status gcsadmm_query(gcsadmm_handle h, int32_t *num_waves, int32_t *lds_bytes, int32_t *num_special,
                             int32_t *num_workgroup_vertices, int32_t *workgroup_lds_bytes)
{
    if (!h) return GCSADMM_ERR_BAD_ARG;
    if (num_waves) *num_waves = h->plan.n_waves();
    if (lds_bytes) *lds_bytes = h->plan.lds_bytes;
    if (num_special) *num_special = h->n_special();
    if (num_workgroup_vertices) *num_workgroup_vertices = h->n_wg();
    if (workgroup_lds_bytes) *workgroup_lds_bytes = h->plan.wg_lds_bytes;
    return GCSADMM_OK;
}

gcsadmm_status gcsadmm_query_workspace(gcsadmm_handle h, int32_t *num_split_vertices, int32_t *split_lds_bytes, int64_t *workspace_bytes)
{
    if (!h) return GCSADMM_ERR_BAD_ARG;
    if (num_split_vertices) *num_split_vertices = h->n_split();
    if (split_lds_bytes) *split_lds_bytes = h->plan.split_lds_bytes;
    if (workspace_bytes) *workspace_bytes = (int64_t)((size_t)h->plan.split_doubles * sizeof(double));
    return GCSADMM_OK;
}

gcsadmm_status gcsadmm_unit_iterations(gcsadmm_handle h, int32_t *out, int32_t capacity, int32_t *count, void *stream)
{
    return handle_entry(h, [&] { return bad_unless(count); }, [&] {
        const auto &g = h->g;
        const int *src = g.d_wave_iters ? g.d_wave_iters.get() : g.d_wg_iters.get();
        const int n = g.d_wave_iters ? h->plan.n_waves() : (g.d_wg_iters ? h->n_wg() : 0);
        *count = n;
        if (n == 0 || !out) return GCSADMM_OK;
        HIPCHK(h, hipStreamSynchronize((hipStream_t)stream));
        HIPCHK(h, hipMemcpy(out, src, sizeof(int) * (size_t)(n < capacity ? n : capacity), hipMemcpyDeviceToHost));
        return GCSADMM_OK;
    });
}

// =================================================================================================
// batch of handles (include/gcsadmm.h): many small problems advance in one set of launches
// =================================================================================================
const char *gcsadmm_batch_last_error(struct gcsadmm_batch_s *b) { return b ? b->err.c_str() : g_create_error.c_str(); }

void gcsadmm_batch_destroy(struct gcsadmm_batch_s *b)
{
    if (!b) return;
    DeviceGuard device_guard_(b->device);      // the owners release on the batch's device
    batch_unbind(b);
    for (gcsadmm_handle h : b->members)
        if (h) h->batches.erase(std::remove(h->batches.begin(), h->batches.end(), b), h->batches.end());
    delete b;
}

gcsadmm_status gcsadmm_batch_create(const gcsadmm_handle *members, int32_t count, struct gcsadmm_batch_s **out)
{
    if (out) *out = nullptr;
    return entry(g_create_error, [&]() -> gcsadmm_status {
        std::unique_ptr<gcsadmm_batch_s> b;
        const gcsadmm_status st = batch_make(members, count, 0, out, b);
        if (st != GCSADMM_OK) return st;
        DeviceGuard device_guard_(b->device);
        return batch_finish(b, device_guard_.err, out);
    });
}

gcsadmm_status gcsadmm_batch_query(struct gcsadmm_batch_s *b, int32_t *wg_members, int32_t *wave_groups, int32_t *wave_members)
{
    return batch_entry(b, [&] { return GCSADMM_OK; }, [&] {      // (host only: the plan's counts)
        const BatchPlan &bp = b->plan;
        if (wg_members) *wg_members = bp.vertex_grid_x > 0 ? (int32_t)bp.wg_members.size() : 0;
        if (wave_groups) *wave_groups = (int32_t)bp.wave_groups.size();
        if (wave_members) *wave_members = (int32_t)std::count_if(bp.wave_grid.begin(), bp.wave_grid.end(), [](int g) { return g > 0; });
        return GCSADMM_OK;
    });
}

gcsadmm_status gcsadmm_batch_query_terminals(struct gcsadmm_batch_s *b, int32_t *term_groups, int32_t *terminals)
{
    return batch_entry(b, [&] { return GCSADMM_OK; }, [&] {      // (host only: the plan's counts)
        const BatchPlan &bp = b->plan;
        int32_t total = 0;
        for (const TermGroup &g : bp.term_groups) total += (int32_t)g.member.size();
        if (term_groups) *term_groups = (int32_t)bp.term_groups.size();
        if (terminals) *terminals = total;
        return GCSADMM_OK;
    });
}

gcsadmm_status gcsadmm_batch_bind(struct gcsadmm_batch_s *b, const gcsadmm_state *states, double *const *traces_dev, void *stream)
{
    BatchPlan bp;      // (made by the checks, taken by the work)
    return batch_entry(b, [&] {
        if (!states) { b->err = "null state array"; return GCSADMM_ERR_BAD_ARG; }
        // the members may have changed since create (a communicator attached): the rules again, then what only a bind can check
        const gcsadmm_status st = batch_plan_of(b->members, b->flags, bp, b->err);
        if (st != GCSADMM_OK) return st;
        for (int i = 0; i < (int)b->members.size(); ++i) {
            gcsadmm_handle h = b->members[i];
            const std::string who = "member " + std::to_string(i) + ": ";
            if (!state_ok(h, &states[i])) { b->err = who + h->err; return GCSADMM_ERR_BAD_ARG; }
            if (h->batch && h->batch != b) { b->err = who + "the handle is bound to another batch (destroy that batch, or bind it to other states, first)"; return GCSADMM_ERR_BAD_ARG; }
        }
        return GCSADMM_OK;
    }, [&] {
        const int count = (int)b->members.size();
        HIPCHK(b, hipStreamSynchronize((hipStream_t)stream));      // launches of an earlier bind may still read the tables
        batch_unbind(b);
        b->plan = bp;
        const size_t vbytes = gcsadmm_wg_batch_entry_bytes(bp.dtype);
        std::vector<char> vtab(vbytes * bp.wg_members.size());
        std::vector<const gcsadmm_control_block *> cbs((size_t)count);
        b->resets.assign((size_t)count, 0u);
        b->states.assign(states, states + count);
        for (int i = 0; i < count; ++i) {
            cbs[i] = b->members[i]->loop.d_cb.get();
            b->resets[i] = b->members[i]->resets;
        }
        for (size_t r = 0; r < bp.wg_members.size(); ++r) {      // row r of the workgroup launch: with the member's closed-form vertices unless a wave launch has them
            const int i = bp.wg_members[r];
            WgLaunchDesc d = make_wg_desc(b->members[i], &states[i], bp.wave_grid[i] == 0);
            d.order = nullptr;      // index order: a batch does no slowest-first reorder (a member of 512 vertices or more has an order buffer)
            gcsadmm_wg_batch_fill(d, vtab.data() + vbytes * r);
        }
        if (!vtab.empty()) HIPCHK(b, hipMemcpy(b->d_vertex_table.get(), vtab.data(), vtab.size(), hipMemcpyHostToDevice));
        const size_t wbytes = wave_batch_entry_bytes(bp.dtype);
        std::vector<char> wtab;
        for (const WaveGroup &g : bp.wave_groups)
            for (int i : g.members) {
                wtab.resize(wtab.size() + wbytes);
                wave_batch_fill(make_launch_desc(b->members[i], &states[i]), bp.dtype, wtab.data() + wtab.size() - wbytes);
            }
        if (!wtab.empty()) HIPCHK(b, hipMemcpy(b->d_wave_table.get(), wtab.data(), wtab.size(), hipMemcpyHostToDevice));
        // the terminals' entries: the member's solo launch as its parameters at this bind make it (cold_start: no warm-start records)
        const size_t tbytes = gcsadmm_terminal_batch_entry_bytes(bp.dtype);
        std::vector<char> ttab;
        for (const TermGroup &g : bp.term_groups)
            for (size_t k = 0; k < g.member.size(); ++k) {
                ttab.resize(ttab.size() + tbytes);
                gcsadmm_terminal_batch_fill(make_term_desc(b->members[g.member[k]], &states[g.member[k]]), g.term[k], ttab.data() + ttab.size() - tbytes);
            }
        if (!ttab.empty()) HIPCHK(b, hipMemcpy(b->d_term_table.get(), ttab.data(), ttab.size(), hipMemcpyHostToDevice));
        HIPCHK(b, hipMemcpy(b->d_cbs.get(), cbs.data(), sizeof(cbs[0]) * cbs.size(), hipMemcpyHostToDevice));
        const gcsadmm_status est = with_state_type(bp.dtype == GCSADMM_F64, [&](auto t) -> gcsadmm_status {
            using T = decltype(t);
            std::vector<EdgeBatchEntry<T>> etab((size_t)count);
            for (int i = 0; i < count; ++i) {
                gcsadmm_handle h = b->members[i];
                etab[i] = EdgeBatchEntry<T>{make_edge_args<T>(h, &states[i]), h->loop.d_cb.get(), h->loop.d_sums.get(), control_params(h), h->loop.d_counters.get(),
                                            traces_dev ? traces_dev[i] : nullptr, h->loop.d_ticket.get(), h->plan.edge_blocks};
            }
            HIPCHK(b, hipMemcpy(b->d_edge_table.get(), etab.data(), sizeof(etab[0]) * etab.size(), hipMemcpyHostToDevice));
            return GCSADMM_OK;
        });
        if (est != GCSADMM_OK) return est;
        for (gcsadmm_handle h : b->members) h->batch = b;
        b->bound = true;
        return GCSADMM_OK;
    });
}

gcsadmm_status gcsadmm_batch_run(struct gcsadmm_batch_s *b, int32_t k, void *stream)
{
    return batch_entry(b, [&] {
        if (k < 0) return GCSADMM_ERR_BAD_ARG;
        if (need_bound(b) != GCSADMM_OK) return GCSADMM_ERR_BAD_ARG;
        for (size_t i = 0; i < b->members.size(); ++i)      // (bound: every member is alive and bound to this batch)
            if (b->members[i]->resets != b->resets[i]) {
                b->err = "member " + std::to_string(i) + ": gcsadmm_reset was called after gcsadmm_batch_bind (bind again: the tables hold the parameters)";
                return GCSADMM_ERR_BAD_ARG;
            }
        return GCSADMM_OK;
    }, [&] {
        gcsadmm_status st = GCSADMM_OK;
        for (int i = 0; i < k && st == GCSADMM_OK; ++i) st = launch_batch_iteration(b, (hipStream_t)stream);
        return st;
    });
}

gcsadmm_status gcsadmm_batch_poll(struct gcsadmm_batch_s *b, int32_t *status, int32_t *it, void *stream)
{
    return batch_entry(b, [&] { return need_bound(b); }, [&] {
        hipStream_t s = (hipStream_t)stream;
        const int count = (int)b->members.size();
        hipLaunchKernelGGL(batch_poll_kernel, dim3((count + 255) / 256), dim3(256), 0, s, b->d_cbs.get(), count, b->d_poll.get());
        HIPCHK(b, hipGetLastError());
        HIPCHK(b, hipMemcpyAsync(b->poll_host.data(), b->d_poll.get(), sizeof(int) * 2 * (size_t)count, hipMemcpyDeviceToHost, s));
        HIPCHK(b, hipStreamSynchronize(s));
        for (int i = 0; i < count; ++i) {
            if (status) status[i] = b->poll_host[i];
            if (it) it[i] = b->poll_host[count + i];
        }
        return GCSADMM_OK;
    });
}

// =================================================================================================
// state transfer (include/gcsadmm.h): a solved state written to a snapshot keyed by stable vertex ids, and read into another graph
// =================================================================================================
gcsadmm_status gcsadmm_export_state(gcsadmm_handle h, const gcsadmm_state *state, const int32_t *vertex_id, gcsadmm_snapshot *snapshot, void *stream)
{
    TransferJob job;
    return handle_entry(h, [&] { return transfer_add_solo(job, h, state, vertex_id, snapshot, true); }, [&] {
        const gcsadmm_status st = transfer_launch(h, h->loop.d_transfer, job, h->dtype, true, (hipStream_t)stream);
        if (st == GCSADMM_OK) transfer_exported(h, snapshot);
        return st;
    });
}

gcsadmm_status gcsadmm_import_state(gcsadmm_handle h, const gcsadmm_state *state, const int32_t *vertex_id, const gcsadmm_snapshot *snapshot, void *stream)
{
    TransferJob job;
    return handle_entry(h, [&] { return transfer_add_solo(job, h, state, vertex_id, snapshot, false); },
                        [&] { return transfer_launch(h, h->loop.d_transfer, job, h->dtype, false, (hipStream_t)stream); });
}

gcsadmm_status gcsadmm_batch_export_state(struct gcsadmm_batch_s *b, const int32_t *const *vertex_ids, gcsadmm_snapshot *const *snapshots, void *stream)
{
    TransferJob job;
    return batch_entry(b, [&] { return transfer_add_batch(b, job, vertex_ids, snapshots, true); }, [&] {
        const gcsadmm_status st = transfer_launch(b, b->d_transfer, job, b->plan.dtype, true, (hipStream_t)stream);
        for (size_t i = 0; st == GCSADMM_OK && i < b->members.size(); ++i)
            if (snapshots[i]) transfer_exported(b->members[i], snapshots[i]);
        return st;
    });
}

gcsadmm_status gcsadmm_batch_import_state(struct gcsadmm_batch_s *b, const int32_t *const *vertex_ids, const gcsadmm_snapshot *const *snapshots, void *stream)
{
    TransferJob job;
    return batch_entry(b, [&] { return transfer_add_batch(b, job, vertex_ids, snapshots, false); },
                       [&] { return transfer_launch(b, b->d_transfer, job, b->plan.dtype, false, (hipStream_t)stream); });
}

} // extern "C"
