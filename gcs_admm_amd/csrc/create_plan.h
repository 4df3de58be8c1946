// create_plan.h -- what gcsadmm_create decides before it allocates anything: the descriptor checks, the program of every
// vertex, the LDS sizes, the wavefront packing and the host-side arrays the handle uploads.  Host-only and HIP-free, so that the
// decisions can be tested on a machine without a GPU (tests/hostemu/plan_emu.cpp, tests/test_create_plan.py).
#pragma once
#include <algorithm>
#include <cmath>
#include <string>
#include <vector>

#include "canonical_box.h"
#include "gcsadmm.h"
#include "state_transfer_core.h"
#include "step_args.h"
#include "vertex_program.h"
#include "warm_start.h"

// sizing functions of the other objects, which own the layouts: vertex_wg.hip (LDS of one workgroup-program vertex with `units` =
// degree + 1; _t512: the 512-thread build, whose reduction area is larger) and terminal_region.hip (work arrays and warm-start record
// of a region terminal)
int gcsadmm_wg_lds_bytes(int n, int units, int facets, bool box = false);     // box: the BOX instantiation's structured layout
int gcsadmm_wg_lds_bytes_t512(int n, int units, int facets, bool box = false);
bool gcsadmm_wg_has_box(int n);                                                // the BOX instantiation exists for this dimension (3, 6)
long long gcsadmm_terminal_ws_doubles(int n, int facets, int live_edges);
long long gcsadmm_terminal_record_doubles(int n, int facets, int live_edges);

namespace gcsadmm_k {

// (EDGE_BLOCK, threads per workgroup of the edge kernel: step_args.h)
constexpr int REORDER_MIN_UNITS = 512;   // launches with fewer units run all at once: no slowest-first dispatch (reorder_kernel, loop_kernels.h)
constexpr int LDS_CU_BYTES = 160 * 1024;

// edges a thread of the edge kernel has in flight at once on LARGE graphs (edge_unroll<T, C>() in edge_step.h); graphs that would not
// fill the chip with such tiles (fewer than 256 workgroups: one per CU) keep one edge per thread
inline int edge_unroll_rt(int dtype, int c, int E)
{
    const int u = dtype == GCSADMM_F32 ? (c <= 7 ? 4 : 2) : (c <= 7 ? 2 : 1);
    return (E + EDGE_BLOCK * u - 1) / (EDGE_BLOCK * u) >= 256 ? u : 1;
}

struct CreatePlan {
    std::vector<int> deg_in;                 // [V] incoming incidences (they precede the outgoing ones)
    std::vector<double> bc;                  // [max(sum m, 1)] centred right-hand sides b - A c
    // closed form (special_vertex.h): point terminals and vertices no flow can cross
    std::vector<int> special_vtx, special_kind;     // kind 1 = source, 2 = target, 0 = no flow
    // terminals that are regions (terminal_region.h): workspace and warm-start record offsets, launch shape
    int n_term = 0, term_vtx[2] = {-1, -1}, term_is_src[2] = {0, 0};
    long long term_ws_off[2] = {0, 0}, term_rec_off[2] = {0, 0}, term_ws_doubles = 0, term_rec_doubles = 0;
    int term_threads = 256, term_lds_doubles = 0;
    // workgroup program (vertex_wg.hip), heaviest sub-problem first
    std::vector<int> wg_vtx;
    int wg_lds_bytes = 0, wg_box = 0, wg_t512 = 0;
    // its split form (gcsadmm_graph_desc.vertex_workspace), 256 threads, same BOX choice: split_vtx[i] has its units at
    // split_off[i] doubles into a device workspace of split_doubles, 256-byte aligned slabs; heaviest first
    std::vector<int> split_vtx;
    std::vector<long long> split_off;
    long long split_doubles = 0;
    int split_lds_bytes = 0;
    // wavefront program (vertex_program.inc): wavefront w holds wave_vtx[wave_slot_ptr[w] .. wave_slot_ptr[w + 1])
    std::vector<int> wave_slot_ptr{0}, wave_vtx;
    int slots_cap = 1, align_rows = 0, store_dl = 0, all_m4 = 0;
    int wave_mm = 1;                         // facet maximum over the wavefront program's vertices (the handle's MM)
    int lds_bytes = 0;                       // LDS per wavefront
    std::vector<long long> warm_ptr;         // [V+1] warm-start record of v: warm + warm_ptr[v] (generic vertices only)
    bool wave_reorder = false, wg_reorder = false;  // slowest-first dispatch buffers
    std::vector<int> prox_vtx;               // gcsadmm_vertex_prox: every vertex but the terminals
    int prox_lds_bytes = 0;
    std::vector<char> col_owned;             // [max(NI, 1)] 1: the state column of an incidence of these vertices
    std::vector<int> col_vertex;             // [max(NI, 1)] vertex of that column, -1: a ghost column
    double nx = 0, nmu = 0;
    int edge_unroll = 1, edge_blocks = 1;
    // gcsadmm_run may run the edge and control steps as the tail of the workgroup program's launch (vertex_wg_kernel.h): one launch
    // per iteration instead of two
    int fused_tail = 0;
    // state transfer (state_transfer_core.h): both ends of every edge as vertices of this handle, from the CSR (-1: an end that is not
    // among them, a cut edge of a partition), and whether the edge list ascends strictly in (tail, head) -- the edge keys of a snapshot
    // then ascend too, which gcsadmm_export_state / gcsadmm_import_state need
    std::vector<int> edge_tail, edge_head;
    int edges_ascending = 0;
    int n_waves() const { return (int)wave_slot_ptr.size() - 1; }
};

// the checks gcsadmm_create makes before it looks for a device
inline gcsadmm_status check_graph_desc(const gcsadmm_graph_desc *g, std::string &err)
{
    auto fail = [&](gcsadmm_status st, const char *msg) { err = msg; return st; };
    if (!g) return fail(GCSADMM_ERR_BAD_ARG, "null descriptor or output pointer");
    if (g->n < 1 || g->n > 8) return fail(GCSADMM_ERR_UNSUPPORTED, "the vertex kernels are instantiated for n = 1 .. 8");
    if (g->num_vertices < 0 || g->num_edges < 0) return fail(GCSADMM_ERR_BAD_ARG, "negative size");
    if (!g->inc_ptr || !g->poly_ptr || (g->num_edges > 0 && (!g->inc_edge || !g->inc_out || !g->edge_inc_tail || !g->edge_inc_head)) ||
        (g->num_vertices > 0 && (!g->poly_A || !g->poly_b || !g->center)))
        return fail(GCSADMM_ERR_BAD_ARG, "null graph array");
    if (g->state_dtype != GCSADMM_F64 && g->state_dtype != GCSADMM_F32) return fail(GCSADMM_ERR_BAD_ARG, "bad state_dtype");
    const int NIo = g->inc_ptr[g->num_vertices];
    if (g->inc_ptr[0] != 0 || NIo < 0 || g->num_incidences < NIo) return fail(GCSADMM_ERR_BAD_ARG, "inconsistent incidence CSR");
    return GCSADMM_OK;
}

// the rest of the descriptor checks and every decision of gcsadmm_create; `g` has passed check_graph_desc
inline gcsadmm_status make_create_plan(const gcsadmm_graph_desc &g, CreatePlan &p, std::string &err)
{
    auto fail = [&](gcsadmm_status st, const char *msg) { err = msg; return st; };
    const int V = g.num_vertices, E = g.num_edges, n = g.n;
    p = CreatePlan();

    // validate CSR, derive deg_in; degree and facet count of every vertex
    std::vector<int> deg(V), fac(V);
    p.deg_in.assign(V, 0);
    int mm_all = 1;
    for (int v = 0; v < V; ++v) {
        const int lo = g.inc_ptr[v], hi = g.inc_ptr[v + 1];
        if (hi < lo) return fail(GCSADMM_ERR_BAD_ARG, "inc_ptr not monotone");
        bool seen_out = false;
        for (int k = lo; k < hi; ++k) {
            if (g.inc_edge[k] < 0 || g.inc_edge[k] >= E) return fail(GCSADMM_ERR_BAD_ARG, "inc_edge out of range");
            if (g.inc_out[k]) seen_out = true;
            else { if (seen_out) return fail(GCSADMM_ERR_BAD_ARG, "incoming incidences must precede outgoing ones"); p.deg_in[v]++; }
        }
        deg[v] = hi - lo;
        fac[v] = g.poly_ptr[v + 1] - g.poly_ptr[v];
        if (fac[v] < n + 1) return fail(GCSADMM_ERR_BAD_ARG, "polytope with fewer than n+1 facets cannot be bounded");
        mm_all = std::max(mm_all, fac[v]);
    }
    for (int e = 0; e < E; ++e)
        if (g.edge_inc_tail[e] < 0 || g.edge_inc_tail[e] >= g.num_incidences || g.edge_inc_head[e] < 0 || g.edge_inc_head[e] >= g.num_incidences)
            return fail(GCSADMM_ERR_BAD_ARG, "edge incidence slot out of range");
    if (g.edge_major_columns != 0 && g.edge_major_columns != 1) return fail(GCSADMM_ERR_BAD_ARG, "edge_major_columns must be 0 or 1");
    if (g.edge_major_columns) {
        if (g.num_incidences != 2 * (int64_t)E) return fail(GCSADMM_ERR_BAD_ARG, "edge-major columns: num_incidences must be 2 num_edges");
        for (int e = 0; e < E; ++e)
            if (g.edge_inc_tail[e] != e || g.edge_inc_head[e] != E + e)
                return fail(GCSADMM_ERR_BAD_ARG, "edge-major columns: edge_inc_tail[e] must be e and edge_inc_head[e] num_edges + e");
    }
    p.edge_tail.assign(E, -1); p.edge_head.assign(E, -1);
    for (int v = 0; v < V; ++v)
        for (int k = g.inc_ptr[v]; k < g.inc_ptr[v + 1]; ++k) (g.inc_out[k] ? p.edge_tail : p.edge_head)[g.inc_edge[k]] = v;
    p.edges_ascending = transfer_edges_ascend(E, p.edge_tail.data(), p.edge_head.data());
    auto poly_A = [&](int v) { return g.poly_A + (size_t)g.poly_ptr[v] * n; };

    // centred right-hand sides b - A c
    const int MT = g.poly_ptr[V];
    p.bc.assign(MT > 0 ? MT : 1, 0.0);
    for (int v = 0; v < V; ++v)
        for (int j = g.poly_ptr[v]; j < g.poly_ptr[v + 1]; ++j) {
            double s = g.poly_b[j];
            for (int k = 0; k < n; ++k) s -= g.poly_A[(size_t)j * n + k] * g.center[(size_t)v * n + k];
            p.bc[j] = s;
            if (v != g.src && v != g.dst && !(s > 0.0)) return fail(GCSADMM_ERR_BAD_ARG, "center is not strictly inside its polytope");
        }

    // ---- classify the vertices ----
    // closed form: s, t (points) and vertices no flow can cross; generic: an interior-point solve each.  A generic vertex
    // goes to the WORKGROUP program (vertex_wg.hip) when the wavefront program cannot take it (n != 2, more than 63
    // incident edges) or when the graph is small enough that latency, not throughput, decides (or on request).
    // s / t: the reference builds them as points (utils.py:12-28, boxes of half-width 1e-6) -> closed form (special_vertex.h).  A terminal
    // whose polytope has an extent is a REGION: its sub-problem is the reference's with delta_sv / delta_tv (admm_solver_v3.py:450-464),
    // solved by terminal_region.h.  Extent = the widest distance from `center` to a facet; the rule the oracle uses (terminal_extent).
    auto live_edges = [&](int v, bool is_src) { return is_src ? deg[v] - p.deg_in[v] : p.deg_in[v]; };
    for (int term : {g.src, g.dst}) {
        if (term < 0 || term >= V) continue;
        double ext = 0;
        for (int j = g.poly_ptr[term]; j < g.poly_ptr[term + 1]; ++j) {
            double nrm = 0;
            for (int k = 0; k < n; ++k) nrm += g.poly_A[(size_t)j * n + k] * g.poly_A[(size_t)j * n + k];
            ext = std::max(ext, std::fabs(p.bc[j]) / std::sqrt(nrm > 0 ? nrm : 1.0));
        }
        if (ext > 1e-5) {
            if (g.src == g.dst) return fail(GCSADMM_ERR_UNSUPPORTED, "source and target are the same region");
            if (live_edges(term, term == g.src) < 1)
                return fail(GCSADMM_ERR_UNSUPPORTED, "a terminal that is a region needs an edge on its live side (outgoing for the source, incoming for the target)");
            p.term_vtx[p.n_term] = term; p.term_is_src[p.n_term] = term == g.src; ++p.n_term;
        }
    }
    auto is_region_terminal = [&](int v) { return (p.n_term > 0 && v == p.term_vtx[0]) || (p.n_term > 1 && v == p.term_vtx[1]); };
    auto is_special = [&](int v) { return v == g.src || v == g.dst || p.deg_in[v] == 0 || deg[v] - p.deg_in[v] == 0; };
    int n_generic = 0;
    for (int v = 0; v < V; ++v) n_generic += !is_region_terminal(v) && !is_special(v);
    // Crossover of the two programs on n = 2 (measured on box lattices, profiles/r02/README.md: 1 024 vertices 3 570 vs 3 030 it/s,
    // 1 444 vertices 2 410 vs 3 060): the workgroup program holds 4 workgroups per CU (102 registers), i.e. 1 024 vertices in one
    // round of ~0.28 ms; the wavefront program packs up to 7 vertices per wavefront and serves up to ~7 000 in one round of 0.33 ms.
    constexpr int WG_AUTO_MAX = 1024;
    if (g.vertex_program < 0 || g.vertex_program > 3) return fail(GCSADMM_ERR_BAD_ARG, "vertex_program must be 0, 1, 2 or 3");
    if (g.vertex_workspace < 0 || g.vertex_workspace > 2) return fail(GCSADMM_ERR_BAD_ARG, "vertex_workspace must be 0, 1 or 2");
    const int ws_mode = g.vertex_workspace;
    const bool prefer_wg = g.vertex_program >= 2 || (g.vertex_program == 0 && n_generic <= WG_AUTO_MAX);
    // box instantiations: the workgroup program's where it has one (n = 3, 6), the wavefront program's at n = 2 (facets
    // [+e0, +e1, -e0, -e1]); wave_generic_rows forces the generic variants of both
    bool wg_box = g.wave_generic_rows == 0 && gcsadmm_wg_has_box(n);
    bool wave_box = n == 2 && g.wave_generic_rows != 1 && g.wave_generic_rows != 2;
    std::vector<int> wave_cand;              // the wavefront program's vertices, in vertex order
    p.warm_ptr.assign(V + 1, 0);             // one warm-start record per generic vertex (either program), none for the closed-form ones
    for (int v = 0; v < V; ++v) {
        p.warm_ptr[v + 1] = p.warm_ptr[v];
        if (is_region_terminal(v)) continue;      // its own kernel
        if (is_special(v)) {
            if (deg[v] > MAX_SPECIAL_DEG) return fail(GCSADMM_ERR_UNSUPPORTED, "terminal vertex degree above 256");
            p.special_vtx.push_back(v);
            p.special_kind.push_back(v == g.src ? 1 : (v == g.dst ? 2 : 0));
            continue;
        }
        p.warm_ptr[v + 1] += gcs_ws::warm_record_doubles(n, fac[v], deg[v]);
        // (vertex_workspace 1: an n = 2 vertex the wavefront program cannot hold even alone in a wavefront goes to the workgroup program)
        const bool wave_too_small = ws_mode == 1 && n == 2 && (size_t)gcs::lds_doubles(n, fac[v], 1, 0) * 8 > (size_t)LDS_CU_BYTES;
        if (n != 2 || deg[v] + 1 > gcs::WAVE || prefer_wg || wave_too_small) {
            p.wg_vtx.push_back(v);
            if (wg_box && !canonical_box(n, fac[v], poly_A(v))) wg_box = false;
        } else {
            wave_cand.push_back(v);
            p.wave_mm = std::max(p.wave_mm, fac[v]);
            if (wave_box && !canonical_box(2, fac[v], poly_A(v))) wave_box = false;
        }
    }

    // ---- workgroup program ----
    // threads per workgroup: 512 while every workgroup of the launch has a CU to itself (vertex_wg_launch.h), 256 otherwise
    const int n_wg = (int)p.wg_vtx.size();
    p.wg_t512 = n_wg > 0 && g.vertex_program != 3 && n_wg + 1 <= 256;
    p.wg_box = n_wg > 0 && wg_box;      // (n_wg: before the split below; both launches take this choice)
    auto wg_bytes = [&](int v) { return p.wg_t512 ? gcsadmm_wg_lds_bytes_t512(n, deg[v] + 1, fac[v], wg_box)
                                                  : gcsadmm_wg_lds_bytes(n, deg[v] + 1, fac[v], wg_box); };
    if (ws_mode > 0) {      // split form: the vertices that do not fit (1) or all of them (2) leave the in-LDS launch
        std::vector<int> keep;
        for (int v : p.wg_vtx) (ws_mode == 2 || wg_bytes(v) > LDS_CU_BYTES ? p.split_vtx : keep).push_back(v);
        p.wg_vtx.swap(keep);
    }
    for (int v : p.wg_vtx) p.wg_lds_bytes = std::max(p.wg_lds_bytes, wg_bytes(v));
    if (p.wg_lds_bytes > LDS_CU_BYTES) return fail(GCSADMM_ERR_UNSUPPORTED, "a vertex sub-problem (degree x facets) does not fit the 160 KB of LDS of a CU");
    // heaviest sub-problems first: the launch ends when its slowest workgroup does
    auto heavier = [&](int a, int b) { return (long)(deg[a] + 1) * fac[a] > (long)(deg[b] + 1) * fac[b]; };
    std::stable_sort(p.wg_vtx.begin(), p.wg_vtx.end(), heavier);
    // split form (256-thread build): LDS = the layout without units, total(0, m); slab = what the units add, rounded to 256 bytes
    std::stable_sort(p.split_vtx.begin(), p.split_vtx.end(), heavier);
    for (int v : p.split_vtx) {
        const int lds = gcsadmm_wg_lds_bytes(n, 0, fac[v], wg_box);
        if (lds > LDS_CU_BYTES) return fail(GCSADMM_ERR_UNSUPPORTED, "a vertex's border system and polytope do not fit the 160 KB of LDS of a CU");
        p.split_lds_bytes = std::max(p.split_lds_bytes, lds);
        p.split_off.push_back(p.split_doubles);
        p.split_doubles += ((gcsadmm_wg_lds_bytes(n, deg[v] + 1, fac[v], wg_box) - lds) / 8 + 31) / 32 * 32;
    }

    // ---- wavefront program: pack its vertices into wavefronts, d+1 lanes each ----
    // LDS per wavefront with / without room for the final dual directions (kernel template SDL): they save the
    // update pass its facet rows (10k lattice +5 %) but must not cost a resident wavefront: kept only while four
    // wavefronts still fit a CU's 160 KB
    auto lds_need = [&](int slots, int store_dl) {
        return (size_t)(wave_box ? gcs_box::lds_doubles(n, p.wave_mm, slots, store_dl) : gcs::lds_doubles(n, p.wave_mm, slots, store_dl)) * 8;
    };
    int slots_max = gcs::MAX_SLOTS;           // vertices a wavefront may take
    if (!wave_cand.empty()) {
        while (slots_max > 1 && lds_need(slots_max, 0) > LDS_CU_BYTES) --slots_max;
        if (lds_need(slots_max, 0) > LDS_CU_BYTES) return fail(GCSADMM_ERR_UNSUPPORTED, "facet count too large for LDS");
        // fewer vertices than wave slots: one vertex per wavefront (a wavefront runs as long as its slowest vertex)
        if (g.wave_slots > 0) slots_max = std::max(1, std::min(slots_max, (int)g.wave_slots));
        else slots_max = std::min(slots_max, std::max(1, ((int)wave_cand.size() + 1023) / 1024));
    }
    // Group placement (vertex_program.inc group_base).  Aligned: no side segment straddles a 16-lane row, the
    // reductions use DPP row shifts (kernel RMODE 0).  Dense: groups back to back, more vertices per wavefront,
    // reductions by chained wave shifts (RMODE 1).  Aligned wins while the wavefronts fit the chip in
    // two rounds (2 x 1024 one-wave-per-SIMD slots); beyond that throughput is per wavefront and dense wins
    // (10k lattice: 1 490 vs 1 440 it/s; 100k lattice: 241 vs 264 it/s).
    auto pack = [&](int align) {
        p.wave_slot_ptr.assign(1, 0); p.wave_vtx.clear();
        int lanes = 0, slots = 0, slots_used = 0;
        for (int v : wave_cand) {
            int base = gcs::group_base(lanes, deg[v], p.deg_in[v], align);
            if (base < 0 || slots + 1 > slots_max) {
                p.wave_slot_ptr.push_back((int)p.wave_vtx.size());
                slots = 0;
                base = gcs::group_base(0, deg[v], p.deg_in[v], align);
            }
            p.wave_vtx.push_back(v);
            lanes = base + deg[v] + 1; slots += 1;
            slots_used = std::max(slots_used, slots);
        }
        if ((int)p.wave_vtx.size() > p.wave_slot_ptr.back()) p.wave_slot_ptr.push_back((int)p.wave_vtx.size());
        p.slots_cap = std::max(1, slots_used);
    };
    pack(1);
    p.align_rows = g.wave_align == 1 ? 1 : (g.wave_align == 2 ? 0 : (p.n_waves() > 2048 ? 0 : 1));
    if (!p.align_rows) pack(0);
    p.all_m4 = wave_box ? 2 : 0;
    if (p.n_waves() > 0) {
        p.store_dl = g.wave_store_dl == 1 ? 1 : (g.wave_store_dl == 2 ? 0 : (lds_need(p.slots_cap, 1) <= 40 * 1024 ? 1 : 0));
        if (p.store_dl && lds_need(p.slots_cap, 1) > LDS_CU_BYTES) p.store_dl = 0;
        p.lds_bytes = (int)lds_need(p.slots_cap, p.store_dl);
    }

    // ---- region terminals: workspace and warm-start records ----
    // the solve is latency-bound: work arrays in LDS while they fit 48 KB, one wavefront (barriers and reductions stay inside it)
    // while no phase has more than four passes over its rows
    long long largest = 0;
    int rows = 0;
    for (int i = 0; i < p.n_term; ++i) {
        const int v = p.term_vtx[i], live = live_edges(v, p.term_is_src[i]);
        const long long need = gcsadmm_terminal_ws_doubles(n, fac[v], live);
        p.term_ws_off[i] = p.term_ws_doubles; p.term_ws_doubles += need; largest = std::max(largest, need);
        p.term_rec_off[i] = p.term_rec_doubles; p.term_rec_doubles += gcsadmm_terminal_record_doubles(n, fac[v], live);
        rows = std::max(rows, live * 2 * fac[v]);
    }
    if (p.n_term > 0) {
        p.term_lds_doubles = largest * 8 <= 48 * 1024 ? (int)largest : 0;
        p.term_threads = rows <= 256 ? 64 : 256;
    }

    p.wave_reorder = p.n_waves() >= REORDER_MIN_UNITS;
    p.wg_reorder = n_wg >= REORDER_MIN_UNITS;
    for (int v = 0; v < V; ++v)
        if (v != g.src && v != g.dst) p.prox_vtx.push_back(v);
    p.prox_lds_bytes = gcsadmm_wg_lds_bytes(n, 1, mm_all);

    // state column of every incidence: owned, and by which vertex
    const size_t ncol = (size_t)std::max<int64_t>(g.num_incidences, 1);
    p.col_owned.assign(ncol, 0);
    p.col_vertex.assign(ncol, -1);
    for (int v = 0; v < V; ++v)
        for (int k = g.inc_ptr[v]; k < g.inc_ptr[v + 1]; ++k) {
            const int col = state_column(g.edge_major_columns, E, 0, k, g.inc_edge[k], g.inc_out[k]);
            p.col_owned[col] = 1; p.col_vertex[col] = v;
        }
    p.nx = g.nx_global > 0 ? g.nx_global : (4.0 * n + 1) * (V + 2.0 * E);
    p.nmu = g.nmu_global > 0 ? g.nmu_global : (4.0 * n + 2) * E;
    p.edge_unroll = edge_unroll_rt(g.state_dtype, 2 * n + 1, E);
    const int tile = EDGE_BLOCK * p.edge_unroll;     // edges per workgroup and pass
    p.edge_blocks = std::max(1, std::min((E + tile - 1) / tile, 2048));
    // FUSED TAIL: all edges fit one edge workgroup; the vertex step is ONE launch of the in-LDS workgroup program (no wavefront
    // program, no split vertices, no region terminal -- its kernel joins from an auxiliary stream after the vertex launch); and the
    // handle is whole (a partition has ghost columns or ownership masks, and its edge step waits for the halo exchange)
    const bool partitioned = g.num_incidences > g.inc_ptr[V] || g.inc_counted != nullptr || g.edge_counted != nullptr;
    p.fused_tail = p.edge_blocks == 1 && E <= EDGE_BLOCK && p.n_waves() == 0 && p.split_vtx.empty() && p.n_term == 0 && !p.wg_vtx.empty() && !partitioned;
    return GCSADMM_OK;
}

}  // namespace gcsadmm_k
