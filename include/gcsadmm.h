/*
 * gcsadmm.h -- C ABI of the MI355X (gfx950) implementation of the per-iteration
 * loop of the reference's "full vertex split" ADMM solver for shortest paths in
 * graphs of convex sets.
 *
 * The reference (Python) has no FFI seam; the call sites this library replaces
 * are, in /root/reference/admm_solver_v3.py:
 *     :469-540  parallel_vertex_update()  -- SolveInParallel(progs, MOSEK) + scatter   -> gcsadmm_vertex_step
 *     :543-587  parallel_edge_update()    -- per-edge average of the two vertex copies \
 *     :590-594  dual_update()             -- mu += A x + B z - c                        > gcsadmm_edge_step
 *     :597-614  residuals, eps_pri/dual   -- the five norms                            /
 *     :655-733  the while loop            -- order, rho adaptation, stop test          -> gcsadmm_control / gcsadmm_run
 * and GCS_utils.py:184-211 compute_cost -> gcsadmm_cost.
 *
 * Conventions
 *   - plain C, no exceptions, no exit(): every entry point returns a gcsadmm_status code;
 *     gcsadmm_last_error() gives the text of the last failure on that handle.
 *   - graph description pointers are HOST pointers (copied at create); state, trace and
 *     scalar buffers are DEVICE pointers owned by the caller (e.g. PyTorch-ROCm tensors).
 *   - one handle <-> one device <-> one stream at a time; calls on a handle are not re-entrant.
 *     `stream` is a hipStream_t passed as void* (NULL = default stream).  All entry points
 *     that take a stream only enqueue work; they never synchronise.
 *
 * State layout (shared with the CPU oracle): for every directed edge e=(u,w) the
 * coupled words are [ z_{e,u}[0:n], z_{e,w}[0:n], y_e ]  (c = 2n+1 words).
 *   copy [c][NI]   vertex copies, incidence-major (word-major rows of NI = incidences)
 *   mu   [c][NI]   scaled duals of the consensus rows, same indexing
 *   zedge[c][E]    edge copies
 *   xv [V][2n], zv [V][2n], yv [V]   per-vertex outputs of the last vertex step
 * Element type of copy/mu/zedge is f64 or f32 (desc.state_dtype); xv/zv/yv are f64.
 * All interior-point arithmetic is f64 regardless.
 */
#ifndef GCSADMM_H
#define GCSADMM_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef enum gcsadmm_status {
    GCSADMM_OK = 0,
    GCSADMM_ERR_BAD_ARG = 1,        /* null pointer, negative size, inconsistent CSR, unsupported n */
    GCSADMM_ERR_UNSUPPORTED = 2,    /* n outside 1 .. 8; a vertex whose sub-problem does not fit the CU's LDS (with vertex_workspace 0)
                                       or whose border system and polytope do not (1, 2); a facet count too large for the wavefront
                                       program (n = 2, vertex_workspace 0); a point terminal of degree above 256; a terminal that is a
                                       region without an edge on its live side, or source and target the same region */
    GCSADMM_ERR_HIP = 3,            /* a HIP runtime call failed */
    GCSADMM_ERR_NO_DEVICE = 4,
    GCSADMM_ERR_NO_MEMORY = 5       /* a host allocation failed ("out of host memory"); never an exception across the ABI */
} gcsadmm_status;

enum { GCSADMM_F64 = 0, GCSADMM_F32 = 1 };

/* loop exit reasons written to gcsadmm_control_block.status */
enum { GCSADMM_RUNNING = -1, GCSADMM_CONVERGED = 0, GCSADMM_MAX_IT = 1, GCSADMM_DIVERGED = 2 };

typedef struct gcsadmm_graph_desc {
    int32_t n;                       /* space dimension: 1 .. 8 */
    int32_t num_vertices;            /* vertices whose sub-problem this handle solves */
    int32_t num_edges;               /* directed edges this handle updates */
    int32_t num_incidences;          /* NI: columns of copy/mu; >= inc_ptr[num_vertices]; the surplus are
                                        ghost slots filled by the caller (halo of a vertex partition) */
    const int32_t *inc_ptr;          /* [V+1] CSR over vertices; incoming edges first, then outgoing */
    const int32_t *inc_edge;         /* [inc_ptr[V]] directed edge id of each incidence */
    const int32_t *inc_out;          /* [inc_ptr[V]] 1 if the vertex is the tail of that edge */
    const int32_t *edge_inc_tail;    /* [E] incidence slot holding the tail's copy of edge e */
    const int32_t *edge_inc_head;    /* [E] incidence slot holding the head's copy */
    const int32_t *poly_ptr;         /* [V+1] CSR over facets */
    const double *poly_A;            /* [poly_ptr[V]][n] facet normals, A x <= b */
    const double *poly_b;            /* [poly_ptr[V]] */
    const double *center;            /* [V][n] a strictly interior point of each polytope */
    int32_t src, dst;                /* local vertex ids of 's' and 't' (-1 if not in this partition).  A terminal whose polytope lies within
                                        1e-5 of its `center` is a point (utils.py:12-28; closed form); one with an extent is a region and is
                                        constrained like any set (admm_solver_v3.py:415-464): own kernel, needs an edge on its live side */
    int32_t state_dtype;             /* GCSADMM_F64 / GCSADMM_F32 */
    int32_t device;                  /* HIP device ordinal */
    const uint8_t *inc_counted;      /* [NI] or NULL(=all 1): this handle owns the copy (counts it in the norms) */
    const uint8_t *edge_counted;     /* [E]  or NULL(=all 1): this handle counts the edge in the norms */
    double nx_global, nmu_global;    /* lengths of the reference's x / mu vectors for eps_pri / eps_dual
                                        (admm_solver_v3.py:605-614); 0 = derive from this handle's sizes */
    /* Schedule of the vertex step (all 0 = automatic).  Two programs solve the same sub-problem with the same
     * interior-point method: the WAVEFRONT program (n = 2, degree <= 63; several vertices per 64-lane wavefront,
     * highest throughput on large graphs) and the WORKGROUP program (any n, degree and facet count that fits LDS;
     * one 256-thread workgroup per vertex, lowest latency: small graphs).  These fields replace what used to be
     * process-global environment knobs; they never change WHAT is computed, only how it is laid out on the chip. */
    int32_t vertex_program;          /* 0 auto, 1 wavefront (where it applies), 2 workgroup, 3 workgroup with 256 threads per workgroup even
                                        where the automatic choice is 512 (launches of at most one workgroup per CU) */
    int32_t wave_slots;              /* wavefront program: vertices per wavefront (0 auto) */
    int32_t wave_align;              /* wavefront program: 0 auto, 1 row-aligned groups, 2 dense packing */
    int32_t wave_store_dl;           /* wavefront program: 0 auto, 1 keep the facet-row dual directions in LDS, 2 recompute */
    int32_t wave_generic_rows;       /* 1 (or 2) = generic facet rows everywhere: the any-facet-count instantiation of the wavefront
                                        program and the generic instantiation of the workgroup program even when every polytope is a
                                        canonical axis-aligned box (tuning / tests) */
    /* Numbering of the state columns (copy / mu are [c][num_incidences]).  0: INCIDENCE-major, column k = position k of the
     * vertex CSR (a vertex's columns are contiguous; edge_inc_tail / edge_inc_head give the two columns of an edge; ghost
     * columns follow the owned ones).  1: EDGE-major, the tail-side column of edge e is e and the head-side column is
     * num_edges + e (num_incidences must be 2 num_edges; edge_inc_tail / edge_inc_head must say exactly that; on a partition
     * the remote side of a cut edge is the ghost).  Edge-major makes the edge step a pure stream (measured 2-3x less HBM
     * traffic) and turns the vertex step's column accesses into gathers, which that latency-bound step does not feel:
     * the layout for large graphs.  Same numbers either way. */
    int32_t edge_major_columns;
    /* Vertex sub-problems larger than LDS.  The workgroup program keeps a vertex's whole sub-problem in the CU's 160 KB of LDS.
     * 0: a vertex whose sub-problem does not fit is refused (GCSADMM_ERR_UNSUPPORTED).  1: such vertices are solved in SPLIT form:
     * the part that grows with the degree (one block per incident edge) lives in a device-memory workspace the handle allocates,
     * LDS keeps the border system and the polytope; every other vertex is placed as with 0.  Also with 1, an n = 2 vertex whose
     * facet count the wavefront program cannot hold goes to the workgroup program.  2: every workgroup-program vertex is solved in
     * split form (tuning / tests).  Same numbers in either form.  gcsadmm_query_workspace reports the split. */
    int32_t vertex_workspace;
} gcsadmm_graph_desc;

typedef struct gcsadmm_params {
    double rho;          /* initial penalty (1)                     admm_solver_v3.py:621 */
    double tau_incr;     /* 2                                        :641 */
    double tau_decr;     /* 2                                        :642 */
    double nu;           /* 10                                       :643 */
    int32_t it_rho_limit;/* rho adapts while it < this (0.1*1000)   :644,703 */
    int32_t max_it;      /* 1000                                     :651 */
    double eps_abs;      /* 1e-4                                     :647 */
    double eps_rel;      /* 1e-3                                     :648 */
    double eps_edge;     /* 1e-4 edge activation penalty             :388 */
    double ipm_tol;      /* barrier parameter at which a vertex solve stops (3e-9: the host default, gcs_admm_amd.IPM_TOL) */
    int32_t ipm_max_iter;/* 60 */
    int32_t cold_start;  /* 0 (default): a vertex solve restarts from the record its previous solve left in the handle's workspace
                            (csrc/warm_start.h; MOSEK at admm_solver_v3.py:490 starts cold -- the minimiser is the same);
                            1: every solve starts from the fixed interior point */
} gcsadmm_params;

typedef struct gcsadmm_state {
    void *copy;   /* [c][NI] */
    void *mu;     /* [c][NI] */
    void *zedge;  /* [c][E]  */
    double *xv;   /* [V][2n] */
    double *zv;   /* [V][2n] */
    double *yv;   /* [V]     */
} gcsadmm_state;

/* Loop state kept on the device so that iterations can be enqueued back to back
 * without host round trips.  Lives in device memory owned by the handle;
 * gcsadmm_read_control copies it out (synchronising the given stream). */
typedef struct gcsadmm_control_block {
    double rho;           /* penalty used by the next vertex step */
    double mu_scale;      /* pending rescale of mu (rho change), applied lazily by the next steps */
    double sums[5];       /* |r|^2, |dz|^2, |copy|^2, |zedge|^2, |mu|^2 of the last edge step */
    double pri, dual, eps_pri, eps_dual;
    int32_t it;           /* iteration counter as the reference reports it (starts at 1) */
    int32_t status;       /* GCSADMM_RUNNING / CONVERGED / MAX_IT / DIVERGED */
    int32_t inner_failures; /* vertex solves of the last step that hit ipm_max_iter */
    int32_t inner_iters;    /* interior-point iterations of the last step, summed over vertices */
} gcsadmm_control_block;

typedef struct gcsadmm_handle_s *gcsadmm_handle;

gcsadmm_status gcsadmm_create(const gcsadmm_graph_desc *desc, gcsadmm_handle *out);
void gcsadmm_destroy(gcsadmm_handle h);
const char *gcsadmm_last_error(gcsadmm_handle h);   /* h may be NULL: error of the calling thread's last failed create */

/* (Re)start the loop: control block := {rho, mu_scale 1, it 1, RUNNING}.  Does not touch the state. */
gcsadmm_status gcsadmm_reset(gcsadmm_handle h, const gcsadmm_params *p, void *stream);

/* x-update: one convex sub-problem per vertex, all vertices of the handle.  Reads zedge, mu and
 * the control block's rho / mu_scale; writes copy (owned incidences only), xv, zv, yv. */
gcsadmm_status gcsadmm_vertex_step(gcsadmm_handle h, const gcsadmm_state *st, void *stream);

/* z-update + dual update + the five partial norms over this handle's edges.  Reads copy (all NI
 * columns: ghost slots must have been filled), updates zedge and mu in place, applies and clears
 * the pending mu rescale, writes sums[5] (f64, device) -- the caller all-reduces them across
 * partitions before gcsadmm_control when the graph is partitioned. */
gcsadmm_status gcsadmm_edge_step(gcsadmm_handle h, const gcsadmm_state *st, double *sums_dev, void *stream);

/* residuals, rho adaptation, stop test, it += 1 (admm_solver_v3.py:697-733) from sums_dev[5];
 * appends {rho, pri, dual, eps_pri, eps_dual, inner_failures} to trace_dev[(it-1)*6 ..] if non-NULL. */
gcsadmm_status gcsadmm_control(gcsadmm_handle h, const double *sums_dev, double *trace_dev, void *stream);

/* Enqueue up to k full iterations (vertex, edge, control) with no host synchronisation; once the
 * stop test fires the remaining enqueued kernels exit immediately. */
gcsadmm_status gcsadmm_run(gcsadmm_handle h, const gcsadmm_state *st, int32_t k, double *trace_dev, void *stream);

/* Small graphs -- all edges in one edge workgroup (at most 256), every generic vertex on the in-LDS workgroup program, no region
 * terminal, no ghost columns or ownership masks -- run an iteration of gcsadmm_run as ONE launch: the last vertex workgroup to finish
 * runs the edge and control steps as the tail of the vertex launch (same numbers bit for bit).  mode 0: two launches per iteration
 * (vertex step; edge + control step); 1: automatic, the default.  Returns 1 when gcsadmm_run fuses on this handle, 0 when it does not
 * (larger graphs, a handle attached to a communicator, mode 0).  Every other entry point keeps its launches. */
int32_t gcsadmm_set_fused_tail(gcsadmm_handle h, int32_t mode);

/* Copy the control block to the host (synchronises `stream`). */
gcsadmm_status gcsadmm_read_control(gcsadmm_handle h, gcsadmm_control_block *out, void *stream);

/* sum_v |z_v[:n] - z_v[n:]| + eps_edge * sum_e y_e over counted edges -> cost_dev[0] (f64, device). */
gcsadmm_status gcsadmm_cost(gcsadmm_handle h, const gcsadmm_state *st, double eps_edge, double *cost_dev, void *stream);

/* Kernel-side facts for benchmarking (any pointer may be NULL): workgroups of the wavefront program and their LDS
 * bytes, closed-form vertices, workgroups (= vertices) of the workgroup program and their LDS bytes. */
gcsadmm_status gcsadmm_query(gcsadmm_handle h, int32_t *num_waves, int32_t *lds_bytes, int32_t *num_special,
                             int32_t *num_workgroup_vertices, int32_t *workgroup_lds_bytes);

/* The split form of the workgroup program (gcsadmm_graph_desc.vertex_workspace; any pointer may be NULL): vertices solved in it, LDS
 * bytes of one of its workgroups, bytes of the device-memory workspace that holds their edge blocks. */
gcsadmm_status gcsadmm_query_workspace(gcsadmm_handle h, int32_t *num_split_vertices, int32_t *split_lds_bytes, int64_t *workspace_bytes);

/* Diagnostics (the split form's vertices are not recorded): Newton iterations of the last vertex step per dispatch unit (wavefronts of the wavefront program: the slowest vertex
 * of each; otherwise workgroups = vertices of the workgroup program), for handles large enough to keep them (>= 512 units: the
 * slowest-first dispatch sorts by them; *count = 0 otherwise).  Synchronises `stream`; copies min(*count, capacity) entries. */
gcsadmm_status gcsadmm_unit_iterations(gcsadmm_handle h, int32_t *out, int32_t capacity, int32_t *count, void *stream);

/* As gcsadmm_run, but every kernel launch is bracketed by HIP events recorded on `stream`; after the
 * k iterations the call synchronises and returns the summed device time (ms) and launch count of the
 * vertex-step kernel(s) and of the edge-step kernel.  For measurement (bench.py roofline). */
gcsadmm_status gcsadmm_run_timed(gcsadmm_handle h, const gcsadmm_state *st, int32_t k, double *trace_dev,
                                 void *stream, float *vertex_ms, int32_t *vertex_launches,
                                 float *edge_ms, int32_t *edge_launches);

/* ---------------------------------------------------------------------------------------------
 * Batches of handles: many small problems advance in one set of launches.  A small graph leaves most of the chip idle (benchmark4:
 * 43 workgroups on 256 CUs) and its workgroup program is bound by dependent latency, so the lever for users with MANY small problems
 * (motion planning: many start / goal queries, many scenes) is occupancy.  A batch is a set of ordinary handles: its launches pick the
 * member by the second grid coordinate and run the device functions of the solo kernels on that member's own arguments, control block,
 * counters, sums and ticket.  Every member therefore stops on its own (the others go on; its workgroups leave at once), and its
 * state, control block and trace are bit for bit those of the same handle driven alone by gcsadmm_run with the same parameters.
 *
 * The handles stay owned by the caller and stay usable on their own while no launch of the batch is in flight.  Destroy the batch before
 * its members; a batch whose member was destroyed first can only be destroyed (gcsadmm_batch_bind refuses it).
 * Call order: gcsadmm_create per member; gcsadmm_batch_create; then per solve gcsadmm_reset on every member, gcsadmm_batch_bind, and
 * gcsadmm_batch_run / gcsadmm_batch_poll until no member is RUNNING; gcsadmm_read_control, gcsadmm_cost etc. per member as usual.
 *
 * Eligibility (checked at create and again at bind; a violation returns GCSADMM_ERR_UNSUPPORTED or GCSADMM_ERR_BAD_ARG and the text
 * names the member and the reason): at least one member, at most 65535, no handle twice, all on one device; the same n and
 * state_dtype; every generic vertex on the in-LDS workgroup program with 256 threads (handles created with vertex_program = 3) and
 * the same BOX choice (all polytopes canonical boxes at n = 3, 6, or not); no vertices on the wavefront program or in the split form,
 * no terminal that is a region, fewer than 512 workgroup-program vertices, an edge step that runs one edge per thread (always the case
 * below 131 072 edges), no communicator attached.  Members may differ in graph, sizes, LDS bytes, column numbering, ownership masks and every
 * field of gcsadmm_params.  Every member keeps its own copy of its graph's polytope data, also where members share a scene.
 *
 * GCSADMM_BATCH_LARGE (gcsadmm_batch_create_ex) lifts two of these rules.  A member may have vertices on the WAVEFRONT program (n = 2,
 * vertex_program = 0 or 1): that program takes a whole SIMD per wavefront, 1 024 on the chip, and a member packed at several vertices
 * per wavefront (wave_slots) fills a fraction of them, so several members share a launch.  The members are grouped by the three plan
 * choices that select a kernel instantiation (box or generic rows, aligned or dense groups, stored dual directions or not) and every
 * group is one launch of vertex_wave_batch_kernel per iteration, which also carries the closed-form vertices of its members.  And a
 * member may have any number of workgroup-program vertices, or both kinds: a batch does no slowest-first reorder, which changes the
 * order of dispatch and never a result.  Per iteration: the workgroup launch over the members that have something in it, one wave
 * launch per group, the edge + control launch.  Everything else above holds, the bit-for-bit statement included.
 *
 * GCSADMM_BATCH_TERMINALS (gcsadmm_batch_create_ex; may be combined with GCSADMM_BATCH_LARGE) lifts "no terminal that is a region".  The
 * region terminals of all members are grouped by the thread count of their solve (64 or 256) and by where its work arrays live (LDS or
 * the handle's workspace), at most four groups, and every group is one launch of terminal_region_batch_kernel per iteration, one
 * workgroup per terminal, on a stream of the batch's own beside the vertex launches.  Each terminal keeps its handle's workspace and
 * warm-start records (none under cold_start, as the parameters at bind say).  Every other rule stands, and so does bit for bit.
 */
typedef struct gcsadmm_batch_s gcsadmm_batch_s;
/* GCSADMM_BATCH_TERMINALS is 4, not 2: flags 2 and 3 have been refused as "unknown batch flag" since gcsadmm_batch_create_ex exists
 * and stay refused, so bit 1 stays undefined. */
enum { GCSADMM_BATCH_LARGE = 1, GCSADMM_BATCH_TERMINALS = 4 };

gcsadmm_status gcsadmm_batch_create(const gcsadmm_handle *members, int32_t count, struct gcsadmm_batch_s **out);
/* gcsadmm_batch_create is this call with flags 0; a bit other than GCSADMM_BATCH_LARGE and GCSADMM_BATCH_TERMINALS is GCSADMM_ERR_BAD_ARG */
gcsadmm_status gcsadmm_batch_create_ex(const gcsadmm_handle *members, int32_t count, int32_t flags, struct gcsadmm_batch_s **out);
/* the launches of an iteration (any pointer may be NULL): members in the workgroup launch, wave launches, members over all wave launches */
gcsadmm_status gcsadmm_batch_query(struct gcsadmm_batch_s *b, int32_t *wg_members, int32_t *wave_groups, int32_t *wave_members);
/* ... and its terminal launches (GCSADMM_BATCH_TERMINALS; either pointer may be NULL): launches, region terminals over all of them */
gcsadmm_status gcsadmm_batch_query_terminals(struct gcsadmm_batch_s *b, int32_t *term_groups, int32_t *terminals);
void gcsadmm_batch_destroy(struct gcsadmm_batch_s *b);
const char *gcsadmm_batch_last_error(struct gcsadmm_batch_s *b);   /* b may be NULL: error of the calling thread's last failed create */

/* After gcsadmm_reset of every member: record each member's state pointers (states[count]), trace pointer (traces_dev[count], device
 * pointers as for gcsadmm_run; the array or any entry may be NULL) and parameters, build the per-member argument tables and upload
 * them once.  Synchronises `stream`.  A member that is bound to another batch is refused until that batch is destroyed or bound anew
 * without it; a gcsadmm_reset of a member after the bind makes gcsadmm_batch_run fail until the batch is bound again. */
gcsadmm_status gcsadmm_batch_bind(struct gcsadmm_batch_s *b, const gcsadmm_state *states, double *const *traces_dev, void *stream);

/* Enqueue up to k iterations of every member that is still RUNNING, with no host synchronisation: per iteration ONE vertex launch and
 * ONE edge + control launch for the whole batch (GCSADMM_BATCH_LARGE: the vertex step is the workgroup launch, if any member has
 * something in it, and one wave launch per group; GCSADMM_BATCH_TERMINALS: and one terminal launch per group).  A member whose stop test has fired is left exactly as it stopped. */
gcsadmm_status gcsadmm_batch_run(struct gcsadmm_batch_s *b, int32_t k, void *stream);

/* status[count] and it[count] of the members' control blocks in one copy (either may be NULL; synchronises `stream`). */
gcsadmm_status gcsadmm_batch_poll(struct gcsadmm_batch_s *b, int32_t *status, int32_t *it, void *stream);

/* ---------------------------------------------------------------------------------------------
 * Replanning: the state of a solved handle, carried to another query graph of the same scene (csrc/state_transfer_core.h has the
 * kernels' contract).  A planner asks almost the same query again every tick; the relaxation is convex, so the loop converges from any
 * state, and from the state of the query before it does so in a fraction of the iterations.  Two graphs of a scene number vertices,
 * edges and state columns differently, so a SNAPSHOT names everything by stable ids the caller gives: vertex_id[V] per handle, int32
 * HOST memory, every id >= 0, strictly ascending with the vertex index.  Edge (u, w) has the key (int64(id[u]) << 32) | id[w]; the keys
 * ascend along the edge list exactly when it ascends in (tail, head), which is decided once, at create.
 *
 * A snapshot is plain DEVICE pointers the caller allocates (as for the state); n and state_dtype are the caller's statement of what it
 * is for.  edge_words holds, word-major, zedge, copy at the tail column, copy at the head column, mu at the tail column, mu at the
 * head column (c = 2n + 1 words each) in the state's element type; the mu words hold fl(mu_scale * mu) with the control block's pending
 * rescale applied (f64 product, rounded once for f32 state).  vertex_words holds xv[2n], zv[2n], yv.  rho[0] is the control block's
 * rho.  Everything else is a copy.
 *
 * export: on entry V and E are the capacities of the snapshot's arrays (each at least the handle's); on return they are the handle's
 * num_vertices and num_edges, the lengths of the two key lists and the strides of the word-major arrays.  One launch writes all of it.
 * import: after gcsadmm_reset (batch: after gcsadmm_batch_bind, before gcsadmm_batch_run).  One launch writes EVERY word of the six state
 * arrays: a destination edge whose key is in the snapshot gets its five groups of words, the mu words as fl(word * r) with
 * r = fl(rho_snapshot / rho_handle), the handle's rho read from its control block as gcsadmm_reset left it (r = 1 is a copy); an edge
 * that is not gets zeros; vertices alike by id.  Not carried: the vertex solves' warm-start records (gcsadmm_reset clears them; the first
 * vertex step of a seeded run starts cold), the trace, the iteration counter, rho itself.
 * The batch calls take vertex_ids[count] and snapshots[count], host arrays of pointers; a null snapshots[i] leaves member i untouched
 * (its vertex_ids[i] may then be null too), and all members are served by one launch, on the states the last bind recorded.
 * Each call uploads its table and the ids, enqueues its one launch on `stream` and synchronises it.
 *
 * GCSADMM_ERR_BAD_ARG, with a text, nothing written, nothing launched: ids that are negative or not strictly ascending; a handle
 * whose edge list is not strictly ascending in (tail, head) or that has ghost columns (num_incidences != 2 num_edges); n or
 * state_dtype of snapshot and handle that differ; on export a snapshot smaller than the handle; a null pointer; a handle that has
 * not been reset, a batch that is not bound. */
typedef struct gcsadmm_snapshot {
    int32_t n, state_dtype;
    int32_t V, E;
    int64_t *edge_key;       /* [E] ascending */
    void *edge_words;        /* [5][c][E] */
    int32_t *vertex_id;      /* [V] ascending */
    double *vertex_words;    /* [4n + 1][V] */
    double *rho;             /* [1] */
} gcsadmm_snapshot;

gcsadmm_status gcsadmm_export_state(gcsadmm_handle h, const gcsadmm_state *state, const int32_t *vertex_id, gcsadmm_snapshot *snapshot, void *stream);
gcsadmm_status gcsadmm_import_state(gcsadmm_handle h, const gcsadmm_state *state, const int32_t *vertex_id, const gcsadmm_snapshot *snapshot, void *stream);
gcsadmm_status gcsadmm_batch_export_state(struct gcsadmm_batch_s *b, const int32_t *const *vertex_ids, gcsadmm_snapshot *const *snapshots, void *stream);
gcsadmm_status gcsadmm_batch_import_state(struct gcsadmm_batch_s *b, const int32_t *const *vertex_ids, const gcsadmm_snapshot *const *snapshots, void *stream);

/* ---------------------------------------------------------------------------------------------
 * The x-update of the reference's OTHER splittings: admm_solver_v1.py:334-383 (shared by v2) solves,
 * per vertex, the border-only problem -- no edge blocks -- whose consensus penalty (:350-367) is a separable quadratic in the
 * vertex's own unknowns:
 *     min |z_v[:n] - z_v[n:]| + 1/2 sum_k q_k (u_k - c_k)^2,  u = (x_v [2n], z_v [2n], y_v),
 *     s.t. A z_i <= y_v b,  A (x_i - z_i) <= (1 - y_v) b  (:371-381),  0 <= y_v <= 1  (:346).
 * Same interior-point method and kernel as the v3 vertex step (workgroup program, "prox" configuration).  q_dev, c_dev:
 * [V][4n+1] f64 device arrays (weights >= 0, not all zero per vertex; centres); outputs [V][2n], [V][2n], [V] f64 device arrays.
 * The two terminals are points (closed form; a graph with a terminal that is a region is refused here).  failures_host (may be NULL; non-NULL synchronises the stream) receives the
 * number of inner solves that did not converge (their outputs are left untouched).  The edge side of those splittings -- one
 * monolithic conic program over all edges (v1) or a sequential sweep (v2) -- is out of scope.
 */
gcsadmm_status gcsadmm_vertex_prox(gcsadmm_handle h, const double *q_dev, const double *c_dev, double *xv_dev, double *zv_dev,
                                   double *yv_dev, double ipm_tol, int32_t ipm_max_iter, int32_t *failures_host, void *stream);

/* ---------------------------------------------------------------------------------------------
 * Vertex partitions across GPUs.  The reference's fan-out point is admm_solver_v3.py:490
 * (SolveInParallel over all vertices); here each rank holds one handle built from its part of the graph (ghost incidence
 * columns for the remote endpoint of every cut edge, ownership masks, global nx / nmu: see gcsadmm_graph_desc) and the ranks
 * meet twice per iteration: the halo exchange of the cut edges' copies and one all-reduce of six doubles.  Both run on the
 * caller's stream through RCCL (bound at run time with dlopen: the library has no link dependency on it).
 */
typedef struct gcsadmm_halo_desc {
    int32_t num_peers;               /* neighbour partitions (<= 2 for strip partitions) */
    const int32_t *peer_rank;        /* [num_peers] */
    const int32_t *send_ptr;         /* [num_peers+1] CSR into send_cols */
    const int32_t *send_cols;        /* owned incidence columns whose copies go to that peer, in (global edge, side) order */
    const int32_t *recv_ptr;         /* [num_peers+1] CSR into recv_cols; recv_ptr == send_ptr entry by entry */
    const int32_t *recv_cols;        /* ghost columns filled from that peer, same canonical order */
} gcsadmm_halo_desc;

/* 128 bytes identifying a new communicator (ncclGetUniqueId); rank 0 calls it, the host distributes the bytes (any transport). */
gcsadmm_status gcsadmm_comm_unique_id(void *id128);

/* Attach rank `rank` of `world` to the communicator `id128` (collective: every rank calls it; blocks until all have) and
 * upload the halo lists.  id128 == NULL: no communicator is created -- for world == 1 the exchange and the all-reduce are
 * no-ops; for world > 1 the host moves the packed halo itself (gcsadmm_halo_pack / _buffers / _unpack) and drives the steps. */
gcsadmm_status gcsadmm_attach_comm(gcsadmm_handle h, int32_t rank, int32_t world, const void *id128, const gcsadmm_halo_desc *halo);
/* The checks gcsadmm_attach_comm makes on the halo lists, alone: host only, no allocation, no collective.  Ranks agree on the outcome
 * (e.g. one all-reduce of an ok flag in the host's own transport) BEFORE any of them enters gcsadmm_attach_comm, whose
 * ncclCommInitRank is collective: a rank that returned an error there would leave its peers waiting. */
gcsadmm_status gcsadmm_check_halo(gcsadmm_handle h, int32_t rank, int32_t world, const gcsadmm_halo_desc *halo);

/* Enqueue up to k full iterations of the partitioned loop (vertex step, halo exchange, edge step, all-reduce, control) with
 * no host synchronisation; every rank must enqueue the same k.  trace_dev as for gcsadmm_run (identical on every rank). */
gcsadmm_status gcsadmm_run_partitioned(gcsadmm_handle h, const gcsadmm_state *st, int32_t k, double *trace_dev, void *stream);

/* As gcsadmm_run_partitioned with every stage bracketed by HIP events on `stream` (collective: every rank calls it with the same k);
 * synchronises and returns the summed device time (ms) of the vertex step, the halo exchange (pack, RCCL send/recv, unpack), the
 * edge step, and the all-reduce + control step.  For measurement (bench.py at N > 1). */
gcsadmm_status gcsadmm_run_partitioned_timed(gcsadmm_handle h, const gcsadmm_state *st, int32_t k, double *trace_dev, void *stream,
                                             float *vertex_ms, float *halo_ms, float *edge_ms, float *reduce_ms);

/* Schedule of gcsadmm_run_partitioned (never its numbers).  The overlapped form ("boundary vertices first") solves the
 * wavefronts that hold a vertex with a cut edge first and on a second stream, with the pack, exchange and unpack of the halo behind them,
 * WHILE the interior wavefronts are solved on the caller's stream; the edge step waits for both.  It exists for handles whose generic vertices all run the
 * wavefront program (the strips of a large n = 2 graph).  mode 0 (default, set at attach): overlapped when the partition has neighbours;
 * 1: overlapped even without neighbours (the first quarter of the wavefronts plays the boundary: tests of the schedule on one GPU);
 * 2: the serial form (vertex step, exchange, edge step on one stream).  boundary_units (may be NULL): wavefronts of the boundary part
 * (0: no split -- the serial form runs).  Call after gcsadmm_attach_comm. */
gcsadmm_status gcsadmm_set_overlap(gcsadmm_handle h, int32_t mode, int32_t *boundary_units);

/* Ranks of the attached RCCL communicator as RCCL itself reports them (ncclCommCount); 0 when none is attached. */
gcsadmm_status gcsadmm_comm_count(gcsadmm_handle h, int32_t *count);

/* The pieces of the halo exchange, for hosts that bring their own transport and for tests: pack the copies to send into the
 * send buffer ([c][columns of peer] per peer, in peer order) / scatter the receive buffer into the ghost columns / both with
 * the RCCL transfer in between / the two device buffers and their length in elements of the state type. */
gcsadmm_status gcsadmm_halo_pack(gcsadmm_handle h, const gcsadmm_state *st, void *stream);
gcsadmm_status gcsadmm_halo_unpack(gcsadmm_handle h, const gcsadmm_state *st, void *stream);
gcsadmm_status gcsadmm_halo_exchange(gcsadmm_handle h, const gcsadmm_state *st, void *stream);
gcsadmm_status gcsadmm_halo_buffers(gcsadmm_handle h, void **send_buf, void **recv_buf, int64_t *num_elements);

/* ---------------------------------------------------------------------------------------------
 * Graph construction at scale.  The reference decides every ordered pair of
 * regions with one LP feasibility solve through Drake/MOSEK (utils.py:31-82 build_graph, :49-65
 * check_overlap); these entry points run the same decisions as batches of tiny LPs on the device, one LP
 * per lane (polytope_lp.hip).  All pointers are HOST pointers (set-up code, called once per scene); the
 * polytope CSR is the one of gcsadmm_graph_desc (rows of region p: poly_ptr[p] .. poly_ptr[p+1]).
 * n = 1..8.  Return value: gcsadmm_status; text of the calling thread's last failure: gcsadmm_polytope_last_error().
 * Optional `status` arrays receive the LP status per problem: 0 converged, 1 / 2 decided early
 * (overlap / separation proven), -1 iteration limit.
 */
const char *gcsadmm_polytope_last_error(void);

/* Chebyshev centre (centre of the largest inscribed ball) and its radius for every region: the strictly
 * interior point the vertex kernel centres a sub-problem on (graph.py chebyshev_center on the host).
 * centers[P][n], radii[P] (may be NULL; capped at 1e6 for unbounded sets; <= 0: no interior). */
int gcsadmm_polytope_centers(int n, int num_polytopes, const int *poly_ptr, const double *poly_A, const double *poly_b,
                             int device, double *centers, double *radii, int *status);

/* Axis-aligned bounding box of every region (2n LPs each, started from `centers`); lo[P][n], hi[P][n];
 * unbounded directions come back near +-1e8. */
int gcsadmm_polytope_bounds(int n, int num_polytopes, const int *poly_ptr, const double *poly_A, const double *poly_b,
                            const double *centers, int device, double *lo, double *hi, int *status);

/* overlap[t] = 1 iff regions pair_a[t] and pair_b[t] share a point (closed sets; inscribed radius of the
 * intersection >= -tol), the decision of utils.py:49-65.  `centers` (may be NULL) only supplies start points. */
int gcsadmm_polytope_overlaps(int n, int num_polytopes, const int *poly_ptr, const double *poly_A, const double *poly_b,
                              const double *centers, long num_pairs, const int *pair_a, const int *pair_b, double tol,
                              int device, unsigned char *overlap, int *status);

/* ---------------------------------------------------------------------------------------------
 * The same pipeline on a RESIDENT scene: the polytope CSR is checked and uploaded once, and the centres, the boxes and the pair
 * list stay on the device from the first LP to the last.  The broad phase -- sort-and-sweep over the first coordinate of the
 * boxes -- runs on the device too (sweep_kernel; csrc/box_sweep_core.h has its contract: the pair list of
 * gcs_admm_amd.scene.candidate_pairs, element for element).  The call order is centers, bounds (or set_boxes), candidate_pairs,
 * overlaps, read_pairs, and from then on add_regions and remove_regions in any order, each leaving a decided scene; a call whose input
 * is not resident yet returns GCSADMM_ERR_BAD_ARG.  All pointers are HOST pointers; every
 * output pointer may be NULL.  Every call works on the scene's device and hands the caller's current device back; calls on one
 * scene are not re-entrant.  Text of the calling thread's last failure: gcsadmm_polytope_last_error().
 */
typedef struct gcsadmm_scene_s *gcsadmm_scene;

/* The checks and the upload of the three entry points above, once. */
int gcsadmm_scene_create(int n, int num_polytopes, const int *poly_ptr, const double *poly_A, const double *poly_b, int device,
                         gcsadmm_scene *out);
void gcsadmm_scene_destroy(gcsadmm_scene s);

/* The centre LPs of gcsadmm_polytope_centers; the centres stay resident.  centers[P][n], radii[P], status[P]. */
int gcsadmm_scene_centers(gcsadmm_scene s, double *centers, double *radii, int *status);

/* The bounds LPs of gcsadmm_polytope_bounds from the resident centres.  A side whose LP reports status < 0 is an interior iterate,
 * a box that is too small: it is opened to -inf / +inf in the resident boxes, and in lo / hi if given.  lo[P][n], hi[P][n],
 * status[P][n][2] = (min, max) per axis. */
int gcsadmm_scene_bounds(gcsadmm_scene s, double *lo, double *hi, int *status);

/* Replace the resident boxes (hosts that have their own; tests).  A NaN, or lo > hi in any coordinate: GCSADMM_ERR_BAD_ARG. */
int gcsadmm_scene_set_boxes(gcsadmm_scene s, const double *lo, const double *hi);

/* Broad phase: the unordered pairs a < b of regions whose boxes, each side moved out by pad, meet; they stay resident.  More than
 * 2^31 - 1 pairs: GCSADMM_ERR_UNSUPPORTED. */
int gcsadmm_scene_candidate_pairs(gcsadmm_scene s, double pad, int64_t *num_pairs);

/* Narrow phase: the decision of gcsadmm_polytope_overlaps for every resident pair, each LP started at the resident centre of the
 * pair's first region.  num_undecided counts the pairs with status < 0, whose flag is not a decision. */
int gcsadmm_scene_overlaps(gcsadmm_scene s, double tol, int64_t *num_overlapping, int64_t *num_undecided);

/* The resident pair list, num_pairs entries each; overlap and status need gcsadmm_scene_overlaps to have run. */
int gcsadmm_scene_read_pairs(gcsadmm_scene s, int *pair_a, int *pair_b, unsigned char *overlap, int *status);

/* The convex restriction along fixed paths through the resident regions (the rounding step after the loop; gcs_admm_amd/rounding.py),
 * all paths of the call side by side, one 64-lane workgroup each (path_restrict_core.h).  Path p visits the k_p >= 1 regions
 * path_poly[path_ptr[p] .. path_ptr[p + 1]) in order and has k_p + 1 points q_0 .. q_k: q_j lies in region j - 1 (j >= 1) and in
 * region j (j <= k_p - 1); the sum of the segment lengths |q_{j+1} - q_j| is minimised.  A terminal that is a point is a region like
 * any other (a box of half-width 1e-6).  start and points hold path p's points at offset (path_ptr[p] + p) * n; start must be strictly
 * inside the rows of every point (the Chebyshev centres of the intersections, for instance).  tol > 0 is the stop on the barrier
 * parameter mu, max_iter >= 0 the limit on Newton iterations.
 * status[p]: 0 converged (mu <= tol); 1 a start point is not strictly inside its rows (treat the path as infeasible); -1 failed
 * (iteration limit, non-finite iterate, vanished step above tol).  cost[p] is the polyline length recomputed from points, inf unless
 * status[p] is 0; iterations[p] the Newton iterations taken.  One path's status never affects another's.  Needs none of the other
 * scene calls to have run.  A region index out of range or a path without regions: GCSADMM_ERR_BAD_ARG; totals beyond 2^31 - 1
 * (rows of one path, point coordinates of the call) or a workspace beyond 2^40 doubles: GCSADMM_ERR_UNSUPPORTED, before anything is
 * allocated. */
int gcsadmm_scene_restrict_paths(gcsadmm_scene s, int num_paths, const int *path_ptr, const int *path_poly, const double *start, double tol,
                                 int max_iter, double *points, double *cost, int *iterations, int *status);

/* Queries on a scene whose graph is decided: the regions under each of num_points points (starts and goals), without a region-region
 * LP.  A point p stands for the box [p - eps, p + eps] (a terminal of a query); region r is listed for it unless some row a_i x <= b_i
 * has a_i.p - b_i > (eps + 2 tol) sum_k |a_ik| + 2^-40 (sum_k |a_ik p_k| + |b_i|), which puts the pair LP's r* below -tol.  A listed
 * hit is of class 1 (IN: p lies in the region, every row with 2^-40 (...) to spare) or 2 (UNDECIDED: within about eps of a facet, or just
 * beyond an acute vertex -- decide these with gcsadmm_polytope_overlaps).  locate_kernel (csrc/point_locate_core.h): one 64-lane
 * workgroup per (chunk of regions, point), a count pass and a fill pass, no atomics; the list is ordered by point, then by region
 * index, and is the same on every run.  It stays resident until the next call.  points[num_points][n] are host doubles.  Needs none of
 * the other scene calls to have run and disturbs none of their resident results.  A NaN or inf coordinate, a negative num_points,
 * eps < 0, tol < 0 or null points: GCSADMM_ERR_BAD_ARG (a list made earlier stays); more than 2^31 - 1 hits:
 * GCSADMM_ERR_UNSUPPORTED, before the list is allocated.  num_points = 0 gives an empty list. */
int gcsadmm_scene_locate_points(gcsadmm_scene s, int num_points, const double *points, double eps, double tol, int64_t *num_hits);

/* The same query for BOXES (a start or goal that is a set): the regions that each of the boxes [lo_q, hi_q] meets, as the same resident
 * hit list (it replaces the one of an earlier locate call of either kind), ordered by box, then by region index, the same on every run.
 * With c = (lo + hi) / 2 and h = (hi - lo) / 2, region r is listed for a box unless some row a_i x <= b_i has
 * a_i.c - b_i > sum_k |a_ik| (h_k + 2 tol) + 2^-40 (sum_k |a_ik c_k| + |b_i|), which puts the pair LP's r* below -tol.  A listed hit is
 * of class 1 (IN: the centre lies in the region) or 2 (UNDECIDED: the region may reach into the box without holding its centre -- decide
 * these with gcsadmm_polytope_overlaps).  locate_box_kernel (csrc/box_locate_core.h), in the shape of locate_kernel.  lo, hi
 * [num_boxes][n] are host doubles.  lo > hi in a coordinate, a NaN or inf bound, a negative num_boxes, tol < 0 or a null pointer:
 * GCSADMM_ERR_BAD_ARG (a list made earlier stays); more than 2^31 - 1 hits: GCSADMM_ERR_UNSUPPORTED, before the list is allocated.
 * num_boxes = 0 gives an empty list. */
int gcsadmm_scene_locate_boxes(gcsadmm_scene s, int num_boxes, const double *lo, const double *hi, double tol, int64_t *num_hits);

/* The resident hit list: the hits of point (or box) q are hit_region / hit_class [hit_ptr[q] .. hit_ptr[q + 1]).  Before a
 * gcsadmm_scene_locate_points or gcsadmm_scene_locate_boxes call has produced a list: GCSADMM_ERR_BAD_ARG. */
int gcsadmm_scene_read_hits(gcsadmm_scene s, int64_t *hit_ptr, int *hit_region, unsigned char *hit_class);

/* The nearest regions of points that may lie in NO region (a state estimate just outside the cover, a goal beyond a wall): for every
 * point the regions within radius[q] of it (null radius: +inf for every point), each with the Euclidean projection of the point onto it.
 * csrc/point_project_core.h has the rule.  With the rows normalised (a^_i = a_i / |a_i|_2, b^_i = b_i / |a_i|_2), region r is a candidate
 * of point p unless some row has a^_i.p - b^_i > radius (1 + 1e-9) + 2^-40 (sum_k |a^_ik p_k| + |b^_i|): the distance to one half-space
 * never exceeds the distance to the region.  The candidates are the resident hit list (project_list_kernel, in the shape of
 * locate_kernel: ordered by point, then region index, the same on every run); it replaces the list of an earlier locate call, and such a
 * call replaces it.  gcsadmm_scene_read_hits returns it with hit_class 1 (INSIDE: no row is violated; the nearest point is p itself,
 * the distance 0) or 2 (everything else).  project_solve_kernel then projects p onto every candidate, one lane per pair, by the dual
 * active-set method of Goldfarb and Idnani (finite, exact up to rounding; at most max_iter steps), and gcsadmm_scene_read_projections
 * returns per hit distance[T], nearest[T][n], iterations[T] and status[T]: 0 solved and distance <= radius; 1 solved, beyond the radius
 * (the entry stays in the list); -1 failed (iteration limit, a non-finite value, no step available: distance and nearest are then not
 * a projection -- decide such a pair on the host).  One pair's status never affects another's.  points[num_points][n] and
 * radius[num_points] are host doubles.  Needs none of the other scene calls to have run and disturbs none of their resident results.
 * A NaN or inf coordinate, a NaN or negative radius (+inf is allowed), a negative num_points, max_iter < 0 or null points:
 * GCSADMM_ERR_BAD_ARG (a list made earlier stays); more than 2^31 - 1 candidates: GCSADMM_ERR_UNSUPPORTED, before the list is
 * allocated.  num_points = 0 gives an empty list.  read_projections on a list that a locate call made, or before any list:
 * GCSADMM_ERR_BAD_ARG. */
int gcsadmm_scene_project_points(gcsadmm_scene s, int num_points, const double *points, const double *radius, int max_iter, int64_t *num_hits);
int gcsadmm_scene_read_projections(gcsadmm_scene s, double *distance, double *nearest, int *status, int *iterations);

/* Through which regions segments run, and whether the regions cover them: is a path still inside the free space after an edit, and
 * which corridor of regions does it take?  Segment q is x(t) = from[q] + t (to[q] - from[q]), t in [0, 1].  csrc/segment_clip_core.h has
 * the rule: per (segment, region) pair the span [t_in, t_out] of the parameters at which the segment lies in the region, every row
 * a_i x <= b_i relaxed by tol sum_k |a_ik| (>= tol |a_i|_2) plus an allowance of 2^-40 (|b_i| + sum_k |a_ik| (|p_k| + |d_k|)) for the rounding
 * of the rule itself; the header derives between which two exact spans every reported span lies.  A pair with a non-empty span is a hit.
 * The hits are the resident hit list (segment_clip_kernel, in the shape of locate_kernel: ordered by segment, then region index, the
 * same on every run); it replaces the list of an earlier locate or project call, and such a call replaces it.  gcsadmm_scene_read_hits
 * returns it with hit_class 1 (WHOLE: t_in == 0 and t_out == 1) or 2 (PART), gcsadmm_scene_read_spans t_in[T] and t_out[T].
 * segment_chain_kernel then sweeps every segment from t = 0: among the hits with t_in <= t < t_out it takes the one of largest t_out
 * (the first in the list among equals) and goes on from there.  gcsadmm_scene_read_cover returns per segment status[q] 0 (COVERED:
 * reach[q] == 1.0 exactly) or 1 (GAP: no hit holds reach[q]) and the chain, the hits taken in order, as positions in the hit list:
 * chain_hit[chain_ptr[q] .. chain_ptr[q + 1]), num_chain entries in all -- the shortest sequence of regions that covers the segment.
 * from[num_segments][n] and to[num_segments][n] are host doubles; a segment with from == to is a point.  Needs none of the other scene
 * calls to have run and disturbs none of their resident results.  A NaN or inf coordinate, a negative num_segments, tol < 0 (or NaN or
 * inf) or a null from / to: GCSADMM_ERR_BAD_ARG (a list made earlier stays); more than 2^31 - 1 hits: GCSADMM_ERR_UNSUPPORTED, before
 * the list is allocated.  num_segments = 0 gives empty lists.  read_spans and read_cover on a list that another kind of call made, or
 * before any list, and read_projections on a clip list: GCSADMM_ERR_BAD_ARG. */
int gcsadmm_scene_clip_segments(gcsadmm_scene s, int num_segments, const double *from, const double *to, double tol, int64_t *num_hits,
                                int64_t *num_chain);
int gcsadmm_scene_read_spans(gcsadmm_scene s, double *t_in, double *t_out);
int gcsadmm_scene_read_cover(gcsadmm_scene s, int *status, double *reach, int64_t *chain_ptr, int *chain_hit);

/* Edits of a scene whose graph is decided (csrc/scene_edit_core.h has the contract): afterwards every resident result -- centres, radii,
 * boxes, statuses, the pair list with its flags and statuses -- is what the call order above gives on a scene created from the edited
 * list of regions, element for element and bit for bit, and restrict_paths and locate_points see the edited regions.  A hit list made
 * before an edit is dropped.
 *
 * add_regions appends num_new regions (poly_ptr[0] = 0, rows of new region p: poly_ptr[p] .. poly_ptr[p+1]) as regions P .. P+num_new-1.
 * It needs centers, bounds (or set_boxes), candidate_pairs and overlaps to have run (otherwise GCSADMM_ERR_BAD_ARG, the text names the
 * missing call), and runs only what is new: num_new centre LPs, 2 n num_new bound LPs (failed sides opened), the new boxes against all
 * boxes (cross_kernel: one 64-lane workgroup per (chunk of boxes, sweeping box), count and fill, no atomics) with the pad given --
 * use that of candidate_pairs --, and the pair LPs of the pairs this finds, each from the centre of its first region.  Their flags and
 * statuses are merged into the pair list; the pairs that were there keep theirs.  centers[num_new][n], radii[num_new],
 * center_status[num_new]; num_new_pairs, num_overlapping and num_undecided count the new pairs.  A region without rows, a zero normal, a
 * centre LP with status < 0 or a radius <= 0: GCSADMM_ERR_BAD_ARG (centers, radii and center_status are filled in the last two cases);
 * more than 2^31 - 1 pairs in all: GCSADMM_ERR_UNSUPPORTED, before the list is allocated.  After any failure the scene is exactly as
 * before.
 *
 * remove_regions takes the regions regions[0 .. num_removed) out; the others keep their order and are renumbered without gaps.  Any
 * state of the scene is accepted, and what is resident is compacted: a pair stays iff both its regions stay.  An index out of range or
 * given twice: GCSADMM_ERR_BAD_ARG, the scene unchanged.  num_pairs_left: length of the pair list afterwards (0 if there is none).
 *
 * read_regions copies the resident centres, radii, boxes and their LP statuses out as they are -- no LP runs (after edits: to see what
 * the scene holds).  centers[P][n], radii[P], center_status[P] need centers to have run, lo[P][n] and hi[P][n] resident boxes;
 * box_status[P][n][2] is that of the bounds LPs (unspecified for boxes that were set by hand). */
int gcsadmm_scene_add_regions(gcsadmm_scene s, int num_new, const int *poly_ptr, const double *poly_A, const double *poly_b,
                              double pad, double tol, double *centers, double *radii, int *center_status,
                              int64_t *num_new_pairs, int64_t *num_overlapping, int64_t *num_undecided);
int gcsadmm_scene_remove_regions(gcsadmm_scene s, int num_removed, const int *regions, int64_t *num_pairs_left);
int gcsadmm_scene_read_regions(gcsadmm_scene s, double *centers, double *radii, int *center_status, double *lo, double *hi, int *box_status);

/* The query graphs of a batch, assembled on the device (csrc/query_graph_core.h has the contract and every closed form): a query graph
 * is the region graph with the few edges of its two terminals merged in, so no entry of it needs a sort.
 *
 * build_region_graph makes the region graph from the resident pair list, and keeps it resident: the directed edges, both directions of
 * every pair with a non-zero flag, sorted by (tail, head) -- gcs_admm_amd.scene.edge_arrays element for element --, row_ptr[P + 1] and
 * for every edge the id of the opposite one.  It needs gcsadmm_scene_overlaps to have run (otherwise GCSADMM_ERR_BAD_ARG).  overlap:
 * num_pairs host flags that take the place of the resident flags for this graph only (a host that decided the pairs with status < 0
 * itself passes its decisions; the resident flags stay as they are), or NULL: the resident flags.  Count, host scan, scatter, then
 * every head to "number of smaller heads in its row": no sort, any degree, the same arrays on every run.  num_edges: E_R.  The graph
 * ends with the next gcsadmm_scene_candidate_pairs or gcsadmm_scene_overlaps and with every add_regions or remove_regions that changes
 * the scene.  A query graph on P regions has at most E_R + 4 P + 2 edges; if twice that exceeds 2^31 - 1: GCSADMM_ERR_UNSUPPORTED,
 * before the graph is allocated (a graph built earlier stays).
 *
 * read_region_graph copies it out: row_ptr[P + 1], edge_tail[E_R], edge_head[E_R], reverse[E_R].  No graph: GCSADMM_ERR_BAD_ARG.
 *
 * query_graphs writes the seven index arrays of gcsadmm_graph_desc for num_queries queries, element for element what
 * gcs_admm_amd.queries.SceneQueries.graphs builds on the host: vertex 0 is the start, 1 the goal, r + 2 region r.  Points
 * 0 .. num_queries-1 are the starts and num_queries .. 2 num_queries-1 the goals; point q lies in the regions
 * term_region[term_ptr[q] .. term_ptr[q+1]), strictly ascending (term_ptr[0] = 0; an empty list is a vertex without edges);
 * st_adjacent[i] is 1 iff the boxes of start and goal i meet.  Query i has E_i = E_R + 2 (a + b) + 2 st_adjacent[i] edges, a and b
 * the lengths of its two lists; edge_off[num_queries + 1] must step by exactly that.  Its edge arrays begin at edge_off[i], its
 * incidence arrays (inc_edge, inc_out) at 2 edge_off[i], its inc_ptr (P + 3 entries) at i (P + 3).  One launch of query_graph_kernel
 * serves chunk_queries queries (0: the library chooses), every entry written once by a plain store; the device workspace is the
 * caller's four small arrays plus 4 (8 E + P + 3) bytes per query of one chunk (at most 65 535), and with chunk_queries = 0 the
 * library keeps that within 256 MiB (or one query, if one is larger).  The result does not depend on chunk_queries.
 * Everything is checked on the host before any launch: no region graph or one from before an edit, term_ptr not non-decreasing, a
 * list that is not strictly ascending or leaves [0, P), a st_adjacent other than 0 or 1, an edge_off that does not step by E_i,
 * negative num_queries or chunk_queries, a null array: GCSADMM_ERR_BAD_ARG; more than 2^31 - 1 hits or 2^30 queries:
 * GCSADMM_ERR_UNSUPPORTED.  A refused call writes no output and changes nothing resident. */
int gcsadmm_scene_build_region_graph(gcsadmm_scene s, const unsigned char *overlap, int64_t *num_edges);
int gcsadmm_scene_read_region_graph(gcsadmm_scene s, int64_t *row_ptr, int *edge_tail, int *edge_head, int *reverse);
int gcsadmm_scene_query_graphs(gcsadmm_scene s, int num_queries, const int64_t *term_ptr, const int *term_region,
                               const unsigned char *st_adjacent, int chunk_queries, const int64_t *edge_off, int *edge_tail, int *edge_head,
                               int *inc_ptr, int *inc_edge, int *inc_out, int *edge_inc_tail, int *edge_inc_head);

/* The informed region set of every query of a batch (csrc/informed_core.h has the rule): the regions an optimal path of query (s, g)
 * can touch lie in the ellipsoid with foci s and g whose major axis is the length of any feasible path.  points[2 num_queries][n]: the
 * starts, then the goals (finite); term_ptr and term_region: exactly those of gcsadmm_scene_query_graphs.
 *
 * region_paths finds one candidate path per query: a shortest path on the resident region graph, an edge weighing the distance
 * between the resident centres of its two regions, from a region r under the start (at distance |s - c_r|) to the region r under the
 * goal that minimises distance + |c_r - g| (the smallest r among equals).  One 256-lane workgroup per query relaxes every vertex from
 * its row in rounds, in place, until a round changes nothing; the result does not depend on the order of the lanes.  Device workspace:
 * 8 P bytes per query of a launch, kept within 256 MiB (or one query).  path_region[num_queries][max_len] receives the path from the
 * start side to the goal side (-1 beyond its length), path_len its length, path_cost the length of the polyline s, centres, g.
 * status: 0 found; 1 no region under the start reaches one under the goal (length 0, cost inf); 2 the path has more than max_len
 * regions (length and cost are reported, no region is); -1 the path could not be read back (regions with identical centres in a
 * cycle).  Needs the region graph (not one from before an edit) and the centres.
 *
 * informed_regions applies a bound: keep[i][r] = 1 iff dist(s_i, box_r) + dist(g_i, box_r) <= bound[i] (1 + 1e-9) on the resident
 * boxes, every side moved out by pad, a side opened to infinity never counting.  For a bound that is the length of a feasible path no
 * region of an optimal path is dropped; bound = inf keeps every region.  keep[num_queries][P]; num_kept[num_queries] (or NULL): the
 * count per query.  Needs the boxes.
 *
 * GCSADMM_ERR_BAD_ARG: a missing result, negative num_queries, max_len < 1, a point that is not finite, a hit list that is not
 * strictly ascending or leaves [0, P), a NaN pad, a NaN or negative bound, a null array.  num_queries = 0 does nothing.  A refused call
 * writes no output and changes nothing resident. */
int gcsadmm_scene_region_paths(gcsadmm_scene s, int num_queries, const double *points, const int64_t *term_ptr, const int *term_region,
                               int max_len, int *path_region, int *path_len, double *path_cost, int *status);
int gcsadmm_scene_informed_regions(gcsadmm_scene s, int num_queries, const double *points, const double *bound, double pad,
                                   unsigned char *keep, int64_t *num_kept);

/* The two calls above for start and goal SETS (csrc/informed_set_core.h has the rule and why it is safe).  A terminal is a box: lo and
 * hi are [2 num_queries][n] each, the start boxes and then the goal boxes, finite, lo <= hi; a point is the box with lo == hi, and on
 * such boxes every output has the bits of the point call.  term_ptr and term_region list the regions that meet each box.
 *
 * region_paths_sets: the path of region_paths with the distance of a centre to the box, sqrt(sum_k max(lo_k - c_k, 0, c_k - hi_k)^2), in
 * the place of |s - c_r| and |c_r - g|.  Its rounds stop early: a relaxation is stored only while it is not above the cheapest goal
 * cost seen so far, so a local query settles in the rounds its own path needs.  Status, path, length and cost are those of the search
 * that runs to the end.
 *
 * informed_regions_sets: keep[i][r] = 1 iff gap(S_i, box_r) + gap(G_i, box_r) <= bound[i] (1 + 1e-9), gap the distance between two
 * boxes, the region's sides moved out by pad.  No region of an optimal path from a point of S_i to a point of G_i is dropped when
 * bound[i] is the length of a feasible one.
 *
 * GCSADMM_ERR_BAD_ARG: what the point calls refuse, and a null lo or hi, lo > hi in a coordinate, a bound that is not finite.
 * num_queries = 0 does nothing.  A refused call writes no output and changes nothing resident. */
int gcsadmm_scene_region_paths_sets(gcsadmm_scene s, int num_queries, const double *lo, const double *hi, const int64_t *term_ptr,
                                    const int *term_region, int max_len, int *path_region, int *path_len, double *path_cost, int *status);
int gcsadmm_scene_informed_regions_sets(gcsadmm_scene s, int num_queries, const double *lo, const double *hi, const double *bound, double pad,
                                        unsigned char *keep, int64_t *num_kept);

/* The query graphs of a batch, each on its own kept regions, assembled on the device (csrc/induced_graph_core.h has the contract): what
 * gcs_admm_amd.queries.SceneQueries.graphs(prune="informed") builds on the host by masking and renumbering the whole edge list per
 * query.  keep[num_queries][P]: any non-zero byte keeps region r for query i; the kept regions are renumbered in scene order (new[r] =
 * number of kept regions below r), P'_i of them.  term_ptr, term_region and st_adjacent: exactly those of gcsadmm_scene_query_graphs,
 * in scene indices; every hit region of a query must be kept.  The graph of query i is that of gcsadmm_scene_query_graphs on the
 * induced region graph of its kept set (E'_R,i directed edges, both ends kept) with the hit lists renumbered: vertex 0 the start, 1
 * the goal, new[r] + 2 kept region r.
 *
 * One 256-lane workgroup per query: an exclusive scan of its P flags in tiles of 256 (shuffles inside a wavefront, one LDS stage
 * across the four, a carry from tile to tile), the kept heads of every kept row counted from that row, a scan over the P'_i kept rows,
 * then every entry written once by a plain store; the reverse edge of an edge comes from the rank of every edge of a kept row among
 * its row's kept heads.  Per query the device reads the P flags and the rows of the kept regions: no pass over all E_R edges, no
 * atomics.  The seven arrays are then written by the closed forms of gcsadmm_scene_query_graphs, unchanged.
 *
 * induced_sizes runs the counts alone: num_kept[i] = P'_i, num_edges[i] = E'_R,i + 2 (a + b) + 2 st_adjacent[i], the sizes the caller
 * lays its arrays out by.  induced_query_graphs repeats the counts and writes the graphs: vertex_off[num_queries + 1] must step by
 * exactly P'_i + 3 and edge_off[num_queries + 1] by num_edges[i]; query i's inc_ptr (P'_i + 3 entries) begins at vertex_off[i], its
 * edge arrays at edge_off[i], its incidence arrays (inc_edge, inc_out) at 2 edge_off[i].  One set of launches serves chunk_queries
 * queries (0: the library chooses: at most 65 535, and as many queries with every region kept as keep workspace and results within
 * 256 MiB, or one).  The result does not depend on chunk_queries.
 *
 * Both calls need the region graph (not one from before an edit).  Decided on the host before any launch: everything
 * gcsadmm_scene_query_graphs refuses in the hit lists, a st_adjacent other than 0 or 1, negative num_queries or chunk_queries, a null
 * array, a hit region whose flag is 0 (the text names the query): GCSADMM_ERR_BAD_ARG; more than 2^31 - 1 hits or 2^30 queries:
 * GCSADMM_ERR_UNSUPPORTED.  Offsets that do not step by the counts: GCSADMM_ERR_BAD_ARG, after the counts (which write to the
 * library's workspace alone) and before anything else.  A refused call writes no output and changes nothing resident.  num_queries =
 * 0 does nothing. */
int gcsadmm_scene_induced_sizes(gcsadmm_scene s, int num_queries, const unsigned char *keep, const int64_t *term_ptr, const int *term_region,
                                const unsigned char *st_adjacent, int *num_kept, int64_t *num_edges);
int gcsadmm_scene_induced_query_graphs(gcsadmm_scene s, int num_queries, const unsigned char *keep, const int64_t *term_ptr, const int *term_region,
                                       const unsigned char *st_adjacent, int chunk_queries, const int64_t *vertex_off, const int64_t *edge_off,
                                       int *edge_tail, int *edge_head, int *inc_ptr, int *inc_edge, int *inc_out, int *edge_inc_tail,
                                       int *edge_inc_head);

/* ---- the candidate paths of the rounding step, drawn on the device (gcs_admm_amd/walks.py; csrc/path_walk_core.h has the rule) ----
 * After the loop, rounding draws s-t walks on the relaxed edge activations y_e.  walk_kernel draws them where the solver left y: one
 * 64-lane workgroup per (walk, problem), the visited set a bitmap in LDS, the draws from a counter-based generator (splitmix64 on
 * (walk, position)), so that every walk is independent of every other: walks 0 .. 15 in one call equal walks 0 .. 7 and 8 .. 15 in two.
 * Walk 0 is the most probable path (the largest activation at every step, the last entry among equals); walk w >= 1 picks out-list
 * entry k with probability proportional to its weight floor(min(y, 2) 2^40) (0 for y <= 0, NaN and heads already on the path).
 * Status of a walk: 0 reached dst, 1 dead end (no entry of positive weight), 2 the path would need more than max_len vertices; the
 * vertices walked so far are returned in every case.
 *
 * B problems, concatenated.  Problem i has vertex_off[i+1]-vertex_off[i] vertices and edge_off[i+1]-edge_off[i] edges; its out_ptr (V_i + 1
 * entries, local offsets 0 .. E_i) starts at out_ptr + vertex_off[i] + i, its out_head / out_edge (local ids) at edge_off[i].  Host pointers,
 * checked (monotone CSR, ids in range, src / dst in range, degree and vertex limits) and uploaded once.  A violation returns
 * GCSADMM_ERR_BAD_ARG; more than 524288 vertices in one problem (the bitmap is 64 KB of LDS) or an out-degree above 2^22 (the total
 * weight of an out-list stays within 64 bits) GCSADMM_ERR_UNSUPPORTED; the text names the problem and the reason. */
typedef struct gcsadmm_walks_s gcsadmm_walks_s;
int gcsadmm_walks_create(int num_problems, const int64_t *vertex_off, const int64_t *edge_off, const int *out_ptr, const int *out_head,
                         const int *out_edge, const int *src, const int *dst, int device, struct gcsadmm_walks_s **out);
void gcsadmm_walks_destroy(struct gcsadmm_walks_s *w);
const char *gcsadmm_walks_last_error(struct gcsadmm_walks_s *w);      /* NULL: the calling thread's last failed create */
/* Walks walk_first .. walk_first + num_walks - 1 of every problem.  y_dev: host array [B] of DEVICE pointers to E_i activations of
 * state_dtype (a row of zedge); seed[B] (the bits are taken as unsigned).  Enqueues on `stream` behind the work that wrote y, then
 * synchronises it.  Host outputs: path_vtx[B][num_walks][max_len] (entries beyond a path's length unspecified), path_len[B][num_walks],
 * status[B][num_walks] (0 / 1 / 2).  num_walks = 0 or no problems: nothing is done.  Negative walk_first or num_walks, max_len < 1, a
 * null array or a null activation pointer: GCSADMM_ERR_BAD_ARG; B * num_walks * max_len above 2^31 - 1 or more than 65535 problems:
 * GCSADMM_ERR_UNSUPPORTED, before anything is allocated.  The object stays usable after a refused call. */
int gcsadmm_walks_sample(struct gcsadmm_walks_s *w, const void *const *y_dev, int state_dtype, const int64_t *seed, int walk_first,
                         int num_walks, int max_len, void *stream, int *path_vtx, int *path_len, int *status);

#ifdef __cplusplus
}
#endif
#endif /* GCSADMM_H */
