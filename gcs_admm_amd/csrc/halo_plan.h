// halo_plan.h -- what a vertex partition decides on the host before anything is uploaded (gcsadmm_attach_comm, gcsadmm_set_overlap):
// what a halo description is refused for, where column j of the send list sits in the packed message, and which wavefronts play the
// boundary in the overlapped loop.  Host-only and HIP-free like create_plan.h, whose plan is its input, so that the rules can be
// tested on a machine without a GPU (tests/hostemu/halo_plan_emu.cpp, tests/test_halo_plan.py).
#pragma once
#include <algorithm>
#include <string>
#include <vector>

#include "create_plan.h"

namespace gcsadmm_k {

// the checks of the halo lists: no allocation, no collective (gcsadmm_check_halo, and the head of gcsadmm_attach_comm).
// col_owned: the plan's, [NI].  The first refusal that applies is the one reported.
inline gcsadmm_status check_halo(const std::vector<char> &col_owned, int NI, int rank, int world, const gcsadmm_halo_desc *hd, std::string &err)
{
    auto fail = [&](const char *msg) { err = msg; return GCSADMM_ERR_BAD_ARG; };
    if (!hd || world < 1 || rank < 0 || rank >= world) return fail("bad communicator arguments");
    const int P = hd->num_peers;
    if (P < 0 || (P > 0 && (!hd->peer_rank || !hd->send_ptr || !hd->recv_ptr || !hd->send_cols || !hd->recv_cols))) return fail("null halo array");
    const int n_send = P ? hd->send_ptr[P] : 0, n_recv = P ? hd->recv_ptr[P] : 0;
    if (n_send != n_recv) return fail("halo lists: a partition sends and receives one column per cut edge and neighbour");
    for (int p = 0; p < P; ++p) {
        const int lo = hd->send_ptr[p], cnt = hd->send_ptr[p + 1] - lo;
        if (cnt < 0 || hd->recv_ptr[p + 1] - hd->recv_ptr[p] != cnt || hd->recv_ptr[p] != lo) return fail("halo lists: send and receive counts per peer must agree");
        if (hd->peer_rank[p] < 0 || hd->peer_rank[p] >= world || hd->peer_rank[p] == rank) return fail("halo lists: bad peer rank");
    }
    for (int j = 0; j < n_send; ++j) {
        if (hd->send_cols[j] < 0 || hd->send_cols[j] >= NI || hd->recv_cols[j] < 0 || hd->recv_cols[j] >= NI) return fail("halo lists: column out of range");
        if (!col_owned[hd->send_cols[j]]) return fail("halo lists: send column is not an owned incidence");
        if (col_owned[hd->recv_cols[j]]) return fail("halo lists: receive column is not a ghost column");
    }
    return GCSADMM_OK;
}

// The packed message: per neighbour one contiguous block [c][columns of that peer], the block of peer p at peer_off[p] * c words.
// base[j] / stride[j]: where word 0 of column j of the flat send list sits, and the distance to its next word (halo_pack_kernel);
// the receiving side has the same layout.  `desc` has passed check_halo.
struct HaloPlan {
    std::vector<int> peers, peer_cnt, peer_off;   // neighbour ranks; columns per peer; first column of each peer's block
    std::vector<int> send_cols;                   // the send list as validated (the overlap split is derived from it)
    int n_send = 0, n_recv = 0;                   // halo columns sent / received per iteration
    std::vector<int> base, stride;                // [max(n_send, 1)]
};
inline HaloPlan make_halo_plan(int c, const gcsadmm_halo_desc *desc)
{
    HaloPlan H;
    const int P = desc->num_peers;
    H.peers.assign(desc->peer_rank, desc->peer_rank + P);
    H.peer_cnt.resize(P); H.peer_off.resize(P);
    H.n_send = P ? desc->send_ptr[P] : 0; H.n_recv = P ? desc->recv_ptr[P] : 0;
    H.send_cols.assign(desc->send_cols, desc->send_cols + H.n_send);
    H.base.resize(std::max(H.n_send, 1)); H.stride.resize(std::max(H.n_send, 1));
    for (int p = 0; p < P; ++p) {
        const int lo = desc->send_ptr[p], cnt = desc->send_ptr[p + 1] - lo;
        H.peer_cnt[p] = cnt; H.peer_off[p] = lo;
        for (int j = 0; j < cnt; ++j) { H.base[lo + j] = lo * c + j; H.stride[lo + j] = cnt; }     // block of peer p: [c][cnt] at lo * c
    }
    return H;
}

// The split of the wavefronts for the overlapped loop: boundary = holds a vertex one of whose columns (send_cols) is sent to a neighbour.
// Only for handles whose generic vertices all run the wavefront program (n_wg = n_split = 0: config 4's strips); mode 1 (tests) splits
// even without neighbours -- the first max(1, n_waves / 4) wavefronts play the boundary -- so that the two launches, the second stream
// and the events can be exercised on one GPU; mode 2 never splits.  ids: the wavefronts, boundary first, then interior, each in
// ascending order; n_wave_b of them are boundary.  Nothing to split (also: fewer than two wavefronts, nothing sent outside mode 1, every
// wavefront on one side): ids empty, n_wave_b = 0.
struct OverlapSplit {
    std::vector<int> ids;
    int n_wave_b = 0;
};
inline OverlapSplit overlap_split(const CreatePlan &p, int V, const std::vector<int> &send_cols, int mode, int n_wg, int n_split)
{
    const int n_waves = p.n_waves(), n_send = (int)send_cols.size();
    if (mode == 2 || n_waves < 2 || n_wg > 0 || n_split > 0) return {};
    if (n_send == 0 && mode != 1) return {};
    std::vector<char> vb((size_t)std::max(V, 1), 0);
    for (int j = 0; j < n_send; ++j) {
        const int v = p.col_vertex[send_cols[j]];
        if (v >= 0) vb[v] = 1;
    }
    OverlapSplit s;
    std::vector<int> ids_i;
    for (int w = 0; w < n_waves; ++w) {
        bool b = (n_send == 0) && w < std::max(1, n_waves / 4);
        for (int q = p.wave_slot_ptr[w]; q < p.wave_slot_ptr[w + 1] && !b; ++q) b = vb[p.wave_vtx[q]] != 0;
        (b ? s.ids : ids_i).push_back(w);
    }
    if (s.ids.empty() || ids_i.empty()) return {};      // nothing to overlap with
    s.n_wave_b = (int)s.ids.size();
    s.ids.insert(s.ids.end(), ids_i.begin(), ids_i.end());
    return s;
}

}  // namespace gcsadmm_k
