// state_transfer_core.h -- carrying the ADMM state of a solved member from one query graph of a scene to another: the bodies of
// state_export_kernel and state_import_kernel (loop_kernels.h, gcsadmm.hip) and of their host build
// (tests/hostemu/state_transfer_emu.cpp; the product path is the kernels).
//
// Two query graphs of one scene number their vertices, edges and state columns differently, so a SNAPSHOT (gcsadmm_snapshot,
// include/gcsadmm.h) names everything by stable vertex ids the caller supplies: vertex v by id[v], edge (u, w) by the key
// (int64(id[u]) << 32) | id[w].  Ids ascend with the vertex index and the edge list ascends in (tail, head), so both key lists of a
// snapshot ascend and the import finds its source by a binary search: no sort, no hash, no atomics.
//
//   export   one lane per edge, consecutive lanes consecutive edges (the word-major rows of zedge and of the snapshot stream; the
//            column accesses are gathers under incidence numbering): the lane writes its key and walks the 5 c words -- zedge, copy at
//            the tail and head columns, mu_scale * mu at both, the pending rescale of the control block applied, the product formed in
//            f64 and rounded once to the state type.  The vertices ride in the trailing workgroups (id, xv, zv, yv); lane 0 of the
//            member's first workgroup writes rho.
//   import   one lane per DESTINATION edge: key from the destination ids, search, then the 5 c words -- the snapshot's for a match
//            (mu words times r = rho_snapshot / rho_member, f64, rounded once: the scaled dual is y / rho), zeros otherwise.  Vertices
//            alike.  With num_incidences = 2 num_edges every state column is one side of one edge, so an import writes every word of
//            the member's six state arrays exactly once, by a plain store.
// Both serve all members of a call in one launch: a table of TransferEntry, the workgroups of member m being block_first[m] ..
// block_first[m + 1); a workgroup finds its member by a search over that prefix (uniform per workgroup).  Bound by memory and by the
// search's dependent loads (log2 E of them per lane), not by arithmetic.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <string>
#include <vector>

#include "gcsadmm.h"

#if defined(__HIPCC__)
#define GCS_ST_HD __host__ __device__ __forceinline__
#else
#define GCS_ST_HD inline
#endif

namespace gcsadmm_k {

constexpr int TRANSFER_BLOCK = 256;      // lanes of a workgroup: edges (or vertices) per workgroup

// one member of a call with its snapshot; the state pointers are of the member's state type (the kernel's T)
struct TransferEntry {
    int c, V, E, NI;                    // the member: words per copy (2 n + 1), vertices, edges, state columns (2 E)
    int snap_V, snap_E;                 // entries of the snapshot's two key lists and the strides of its word-major arrays
    int block_first, edge_blocks;       // first workgroup of the member in the launch; its first edge_blocks take edges, the rest vertices
    const int *edge_tail, *edge_head;               // [E] both ends of every edge, vertex indices
    const int *edge_inc_tail, *edge_inc_head;       // [E] state columns of both sides; null: edge-major numbering (e, E + e)
    const int *vertex_id;                           // [V] the member's ids
    void *copy, *mu, *zedge;                        // [c][NI], [c][NI], [c][E]
    double *xv, *zv, *yv;                           // [V][2 n], [V][2 n], [V]
    const gcsadmm_control_block *cb;                // the member's: rho, mu_scale
    int64_t *edge_key;                              // the snapshot: [snap_E]
    void *edge_words;                               // [5][c][snap_E]
    int *snap_vertex_id;                            // [snap_V]
    double *vertex_words;                           // [4 n + 1][snap_V]
    double *snap_rho;                               // [1]
};

GCS_ST_HD int transfer_blocks(int count) { return (count + TRANSFER_BLOCK - 1) / TRANSFER_BLOCK; }
GCS_ST_HD int64_t transfer_key(int id_tail, int id_head) { return (int64_t)(((uint64_t)(uint32_t)id_tail << 32) | (uint64_t)(uint32_t)id_head); }
GCS_ST_HD int transfer_tail_col(const TransferEntry &e, int edge) { return e.edge_inc_tail ? e.edge_inc_tail[edge] : edge; }
GCS_ST_HD int transfer_head_col(const TransferEntry &e, int edge) { return e.edge_inc_head ? e.edge_inc_head[edge] : e.E + edge; }
// a scaled dual is y / rho: one made at rho_snapshot reads at rho_member as itself times this
GCS_ST_HD double transfer_ratio(double rho_snapshot, double rho_member) { return rho_snapshot / rho_member; }

// position of `key` in the ascending list keys[0 .. count), -1 if it is not there
template <class K> GCS_ST_HD int transfer_find(const K *keys, int count, K key)
{
    int lo = 0, hi = count - 1;
    while (lo <= hi) {
        const int mid = lo + (hi - lo) / 2;
        const K k = keys[mid];
        if (k == key) return mid;
        if (k < key) lo = mid + 1;
        else hi = mid - 1;
    }
    return -1;
}

// the member whose workgroups hold `block`: the last entry with block_first <= block (every entry has at least one workgroup)
GCS_ST_HD int transfer_member(const TransferEntry *table, int count, int block)
{
    int lo = 0, hi = count - 1;
    while (lo < hi) {
        const int mid = lo + (hi - lo + 1) / 2;
        if (table[mid].block_first <= block) lo = mid;
        else hi = mid - 1;
    }
    return lo;
}

// ---- export ----
template <class T> GCS_ST_HD void transfer_export_edge(const TransferEntry &e, int edge, double mu_scale)
{
    const size_t E = (size_t)e.E, NI = (size_t)e.NI, plane = (size_t)e.c * E;
    const size_t from_tail = (size_t)transfer_tail_col(e, edge), from_head = (size_t)transfer_head_col(e, edge);
    const T *zedge = (const T *)e.zedge, *copy = (const T *)e.copy, *mu = (const T *)e.mu;
    T *out = (T *)e.edge_words;
    e.edge_key[edge] = transfer_key(e.vertex_id[e.edge_tail[edge]], e.vertex_id[e.edge_head[edge]]);
    for (int w = 0; w < e.c; ++w) {
        const size_t at = (size_t)w * E + (size_t)edge, row = (size_t)w * NI;
        out[at] = zedge[at];
        out[plane + at] = copy[row + from_tail];
        out[2 * plane + at] = copy[row + from_head];
        out[3 * plane + at] = (T)(mu_scale * (double)mu[row + from_tail]);
        out[4 * plane + at] = (T)(mu_scale * (double)mu[row + from_head]);
    }
}

template <class T> GCS_ST_HD void transfer_export_vertex(const TransferEntry &e, int v)
{
    const int n2 = e.c - 1;      // 2 n
    const size_t V = (size_t)e.V;
    e.snap_vertex_id[v] = e.vertex_id[v];
    for (int k = 0; k < n2; ++k) {
        e.vertex_words[(size_t)k * V + (size_t)v] = e.xv[(size_t)v * n2 + k];
        e.vertex_words[(size_t)(n2 + k) * V + (size_t)v] = e.zv[(size_t)v * n2 + k];
    }
    e.vertex_words[(size_t)(2 * n2) * V + (size_t)v] = e.yv[v];
}

// lane `lane` of workgroup `block` of the member (block counted from the member's first)
template <class T> GCS_ST_HD void transfer_export_lane(const TransferEntry &e, int block, int lane)
{
    if (block == 0 && lane == 0) e.snap_rho[0] = e.cb->rho;
    const int i = (block < e.edge_blocks ? block : block - e.edge_blocks) * TRANSFER_BLOCK + lane;
    if (block < e.edge_blocks) {
        if (i < e.E) transfer_export_edge<T>(e, i, e.cb->mu_scale);
    } else if (i < e.V) transfer_export_vertex<T>(e, i);
}

// ---- import ----
template <class T> GCS_ST_HD void transfer_import_edge(const TransferEntry &e, int edge, double ratio)
{
    const size_t E = (size_t)e.E, NI = (size_t)e.NI, SE = (size_t)e.snap_E, plane = (size_t)e.c * SE;
    const size_t to_tail = (size_t)transfer_tail_col(e, edge);
    const size_t to_head = (size_t)transfer_head_col(e, edge);
    T *zedge = (T *)e.zedge, *copy = (T *)e.copy, *mu = (T *)e.mu;
    const T *in = (const T *)e.edge_words;
    const int s = transfer_find(e.edge_key, e.snap_E, transfer_key(e.vertex_id[e.edge_tail[edge]], e.vertex_id[e.edge_head[edge]]));
    const int words = e.c;      // matched or not: every word of the edge is written
    for (int w = 0; w < words; ++w) {
        T z = 0, cu = 0, cw = 0, mu_u = 0, mu_w = 0;
        if (s >= 0) {
            const size_t at = (size_t)w * SE + (size_t)s;
            z = in[at]; cu = in[plane + at]; cw = in[2 * plane + at];
            mu_u = (T)((double)in[3 * plane + at] * ratio);
            mu_w = (T)((double)in[4 * plane + at] * ratio);
        }
        const size_t row = (size_t)w * NI;
        zedge[(size_t)w * E + (size_t)edge] = z;
        copy[row + to_tail] = cu; copy[row + to_head] = cw;
        mu[row + to_tail] = mu_u; mu[row + to_head] = mu_w;
    }
}

template <class T> GCS_ST_HD void transfer_import_vertex(const TransferEntry &e, int v)
{
    const int n2 = e.c - 1;
    const size_t SV = (size_t)e.snap_V;
    const int s = transfer_find(e.snap_vertex_id, e.snap_V, e.vertex_id[v]);
    for (int k = 0; k < n2; ++k) {
        e.xv[(size_t)v * n2 + k] = s >= 0 ? e.vertex_words[(size_t)k * SV + (size_t)s] : 0.0;
        e.zv[(size_t)v * n2 + k] = s >= 0 ? e.vertex_words[(size_t)(n2 + k) * SV + (size_t)s] : 0.0;
    }
    e.yv[v] = s >= 0 ? e.vertex_words[(size_t)(2 * n2) * SV + (size_t)s] : 0.0;
}

template <class T> GCS_ST_HD void transfer_import_lane(const TransferEntry &e, int block, int lane)
{
    const int i = (block < e.edge_blocks ? block : block - e.edge_blocks) * TRANSFER_BLOCK + lane;
    if (block < e.edge_blocks) {
        if (i < e.E) transfer_import_edge<T>(e, i, transfer_ratio(e.snap_rho[0], e.cb->rho));
    } else if (i < e.V) transfer_import_vertex<T>(e, i);
}

// ---- the host side of a call: its checks and its table (gcsadmm.hip; the host build runs the same) ----
// what the checks and the entry read of a handle
struct TransferHandle {
    int n, dtype, V, E, NI, edge_major, edges_ascending;
    bool reset;                                     // gcsadmm_reset has run: the control block holds rho and mu_scale
    const int *edge_tail, *edge_head, *edge_inc_tail, *edge_inc_head;
    const gcsadmm_control_block *cb;
};
// decided once, at create (create_plan.h): both ends of every edge are vertices of the handle and the list ascends strictly in (tail, head)
inline int transfer_edges_ascend(int E, const int *tail, const int *head)
{
    for (int e = 0; e < E; ++e) {
        if (tail[e] < 0 || head[e] < 0) return 0;
        if (e > 0 && !(tail[e - 1] < tail[e] || (tail[e - 1] == tail[e] && head[e - 1] < head[e]))) return 0;
    }
    return 1;
}
// one call: the table of its members and their vertex ids back to back
struct TransferCall {
    std::vector<TransferEntry> table;
    std::vector<int32_t> ids;
    std::vector<size_t> ids_at;      // where the ids of table[i] begin
    int blocks = 0;
};

// The checks of one member (`who`: how the text names it) and, when they pass, its entry (vertex_id is set once the ids have a home).
// A refusal is GCSADMM_ERR_BAD_ARG with its text in `err`, and leaves `call` as it was.
inline gcsadmm_status transfer_add(TransferCall &call, const TransferHandle &h, const gcsadmm_state *st, const int32_t *vertex_id, const gcsadmm_snapshot *snap,
                                   bool exporting, const std::string &who, std::string &err)
{
    auto refuse = [&](const char *msg) { err = who + msg; return GCSADMM_ERR_BAD_ARG; };
    if (!st || !st->copy || !st->mu || !st->zedge || !st->xv || !st->zv || !st->yv) return refuse("null state pointer");
    if (!h.reset) return refuse("gcsadmm_reset has not been called");
    if (!vertex_id || !snap) return refuse("null vertex_id or snapshot");
    if (!snap->edge_key || !snap->edge_words || !snap->vertex_id || !snap->vertex_words || !snap->rho) return refuse("null snapshot array");
    if (snap->n != h.n || snap->state_dtype != h.dtype) return refuse("n or state_dtype of the snapshot differs from the handle's");
    if (snap->V < 0 || snap->E < 0) return refuse("negative snapshot size");
    if (h.NI != 2 * (int64_t)h.E) return refuse("the handle has ghost columns (num_incidences != 2 num_edges)");
    if (!h.edges_ascending) return refuse("the handle's edge list is not strictly ascending in (tail, head)");
    if (exporting && (snap->V < h.V || snap->E < h.E)) return refuse("the snapshot is smaller than the handle");
    for (int v = 0; v < h.V; ++v)
        if (vertex_id[v] < 0 || (v > 0 && vertex_id[v - 1] >= vertex_id[v])) return refuse("vertex ids must be >= 0 and strictly ascending");
    TransferEntry e{};
    e.c = 2 * h.n + 1; e.V = h.V; e.E = h.E; e.NI = h.NI;
    e.snap_V = exporting ? h.V : snap->V; e.snap_E = exporting ? h.E : snap->E;
    e.block_first = call.blocks; e.edge_blocks = transfer_blocks(h.E);
    e.edge_tail = h.edge_tail; e.edge_head = h.edge_head;
    e.edge_inc_tail = h.edge_major ? nullptr : h.edge_inc_tail; e.edge_inc_head = h.edge_major ? nullptr : h.edge_inc_head;
    e.copy = st->copy; e.mu = st->mu; e.zedge = st->zedge; e.xv = st->xv; e.zv = st->zv; e.yv = st->yv;
    e.cb = h.cb;
    e.edge_key = snap->edge_key; e.edge_words = snap->edge_words; e.snap_vertex_id = snap->vertex_id; e.vertex_words = snap->vertex_words; e.snap_rho = snap->rho;
    call.ids_at.push_back(call.ids.size());
    call.ids.insert(call.ids.end(), vertex_id, vertex_id + h.V);
    call.table.push_back(e);
    const int blocks = e.edge_blocks + transfer_blocks(h.V);
    call.blocks += blocks > 0 ? blocks : 1;
    return GCSADMM_OK;
}

}  // namespace gcsadmm_k
