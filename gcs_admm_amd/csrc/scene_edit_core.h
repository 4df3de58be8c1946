// scene_edit_core.h -- adding regions to and removing regions from a resident scene whose graph is decided: the pieces shared by the
// edit kernels (polytope_lp.hip) and their host build (tests/hostemu/scene_edit_emu.cpp; the product path is the kernels).
//
// Contract: after an edit the pair list is the list scene.candidate_pairs gives on the edited set of boxes, element for element, and
// every pair that was there before keeps its flag and status.  box_sweep_core.h has the order: the boxes in stable order of lo[:, 0]
// ("rank"), a pair filed under its earlier box, the pairs of a box by the rank of the later one.
//
// Add (P resident boxes in sweep order, K appended ones with indices P .. P+K-1 in sweep order of their own):
//   ranks   resident box at position i:  i + #(appended with lo0 <  its lo0)      an appended box sorts after a resident one with an
//           appended box at position a:  a + #(resident with lo0 <= its lo0)      equal key, as its larger index demands; -0.0 == +0.0
//   cross   the new pairs, by who sweeps: an appended box over the merged boxes behind it (side F), a resident box over the appended
//           boxes behind it (side B).  One 64-lane workgroup per (chunk of EDIT_CHUNK targets, sweeping box), the window of
//           sweep_kernel clipped to the chunk, the test of sweep_test; the hits of a stride are compacted in lane order (ballot +
//           prefix count) and the (box, chunk) cells are placed by an exclusive scan: no atomics, the same list on every run.  Both
//           sides list the hits of one box by ascending rank of the later box, so the merge needs no sort.
//   merge   new count of a box = its old pairs + its cross pairs; an exclusive scan of those places the boxes; an old pair moves to
//           (its place among the old pairs of its box) + (cross pairs of that box whose later box ranks lower), a cross pair the other
//           way round: two binary searches, every pair written once.
// Remove: regions keep their relative order, so the sweep order, and with it the pair list, is the old one with the removed boxes and
// their pairs left out and the indices renumbered: a count and a fill pass per box of the old sweep order.
#pragma once
#include "box_sweep_core.h"

// targets per workgroup of the cross sweep: a multiple of the wavefront (profiles/scene_edit/README.md has what it was measured against)
#ifndef GCS_EDIT_CHUNK
#define GCS_EDIT_CHUNK 256
#endif

namespace gcsadmm_lp {

constexpr int EDIT_CHUNK = GCS_EDIT_CHUNK;
static_assert(EDIT_CHUNK > 0 && EDIT_CHUNK % SWEEP_WAVE == 0, "a chunk is whole strides");

inline long long edit_chunks(long long count) { return (count + EDIT_CHUNK - 1) / EDIT_CHUNK; }

// numpy.searchsorted(v, key, side="left"): the first index whose value is not below key
GCS_SWEEP_HD int edit_lower_bound(const double *v, int count, double key)
{
    int a = 0, b = count;
    while (a < b) {
        const int mid = a + ((b - a) >> 1);
        if (v[mid] < key) a = mid + 1;
        else b = mid;
    }
    return a;
}

// ---- ranks ----
struct EditRanks {
    int P, K;
    const double *slo0, *alo0;      // first lower bounds in sweep order: resident [P], appended [K]
    const int *order, *aorder;      // region of position i; appended box (0 .. K-1) of position a
    int *arank;                     // merged rank of appended position a
    int *norder, *inv, *oldpos;     // [P+K]: region of rank r; rank of region; who holds rank r: resident position i, or -1 - a
};
// thread t of P + K
GCS_SWEEP_HD void edit_rank(const EditRanks &E, int t)
{
    int r, region;
    if (t < E.P) {
        r = t + edit_lower_bound(E.alo0, E.K, E.slo0[t]);
        region = E.order[t];
        E.oldpos[r] = t;
    } else {
        const int a = t - E.P;
        r = a + sweep_window_end(E.slo0, E.P, E.alo0[a]);
        region = E.P + E.aorder[a];
        E.arank[a] = r;
        E.oldpos[r] = -1 - a;
    }
    E.norder[r] = region;
    E.inv[region] = r;
}

// ---- cross sweep ----
struct CrossSide {
    SortedBoxes S, T;               // the sweeping boxes and their targets, each in sweep order
    const int *srank;               // side F: merged rank of sweeper k (its targets are the merged boxes: the window starts behind it);
                                    // side B: nullptr (the targets are the appended boxes: the window starts at the first one not below)
    const int *trank;               // side B: merged rank of target j; side F: nullptr (the position is the rank)
    const int *norder;              // region of merged rank r
    long long chunks, limit;        // chunks of the targets; length of the list
    int first;                      // blockIdx.y counts sweepers from here
    int *count;                     // [sweepers][chunks], at cell0
    const long long *offset;
    long long cell0;                // first cell of this side in count / offset
    int *rank_e, *rank_l, *pair_a, *pair_b;      // fill: ranks of the earlier and the later box, regions a < b
};

template <int N> GCS_SWEEP_HD void cross_window(const CrossSide &c, int k, const SweepBox<N> &bk, int &w0, int &w1)
{
    w0 = c.srank ? c.srank[k] + 1 : edit_lower_bound(c.T.lo, c.T.P, bk.lo[0]);
    w1 = sweep_window_end(c.T.lo, c.T.P, bk.hip[0]);
}
// does the workgroup of `chunk` see any of the window?
GCS_SWEEP_HD bool cross_chunk_live(long long chunk, int w0, int w1)
{
    return chunk * EDIT_CHUNK < w1 && (chunk + 1) * EDIT_CHUNK > w0;
}
// one lane's target in one stride, and whether it pairs with the sweeper
template <int N> GCS_SWEEP_HD bool cross_hit(const CrossSide &c, const SweepBox<N> &bk, int w0, int w1, long long chunk, int stride, int lane,
                                             double pad, int &j)
{
    const long long at = chunk * EDIT_CHUNK + (long long)stride * SWEEP_WAVE + lane;
    j = (int)at;
    return at >= w0 && at < w1 && sweep_test<N>(c.T, bk, j, pad);
}
// rank of sweeper k whose window starts at w0
GCS_SWEEP_HD int cross_sweeper_rank(const CrossSide &c, int k, int w0) { return c.srank ? c.srank[k] : k + w0; }
GCS_SWEEP_HD void cross_store(const CrossSide &c, long long pos, int re, int j)
{
    if (pos >= c.limit) return;      // (the count pass ran the same tests, so no position reaches it)
    const int rl = c.trank ? c.trank[j] : j;
    c.rank_e[pos] = re;
    c.rank_l[pos] = rl;
    sweep_store_pair(c.pair_a, c.pair_b, pos, c.norder[re], c.norder[rl]);
}

// ---- merge ----
struct EditMerge {
    int P, K;
    long long T_old, T_new;         // resident pairs, cross pairs
    long long chunks_f, chunks_b;   // cells of side F: [K][chunks_f] from 0; of side B: [P][chunks_b] behind them
    const long long *cell_off;      // [cells + 1] exclusive scan of the cross counts
    const int *oldpos, *inv;
    const int *count_old;           // [P] by resident position
    const long long *offset_old;
    const int *pa_old, *pb_old, *st_old;
    const unsigned char *flag_old;
    const int *rank_e, *rank_l, *pa_new, *pb_new, *st_new;
    const unsigned char *flag_new;
    int *count;                     // [P+K] by merged rank
    const long long *offset;
    int *pa, *pb, *st;              // the merged list
    unsigned char *flag;
};
GCS_SWEEP_HD long long merge_cross_begin(const EditMerge &m, int holder)      // holder: oldpos[rank]
{
    return holder >= 0 ? m.cell_off[(long long)m.K * m.chunks_f + (long long)holder * m.chunks_b] : m.cell_off[(long long)(-1 - holder) * m.chunks_f];
}
GCS_SWEEP_HD long long merge_cross_end(const EditMerge &m, int holder)
{
    return holder >= 0 ? m.cell_off[(long long)m.K * m.chunks_f + (long long)(holder + 1) * m.chunks_b]
                       : m.cell_off[(long long)(-holder) * m.chunks_f];
}
// thread r of P + K: pairs filed under the box of merged rank r
GCS_SWEEP_HD void merge_count(const EditMerge &m, int r)
{
    const int holder = m.oldpos[r];
    m.count[r] = (int)(merge_cross_end(m, holder) - merge_cross_begin(m, holder)) + (holder >= 0 ? m.count_old[holder] : 0);
}
GCS_SWEEP_HD int merge_min(int a, int b) { return a < b ? a : b; }
GCS_SWEEP_HD int merge_max(int a, int b) { return a < b ? b : a; }
// thread t of T_old: resident pair t to its new place
GCS_SWEEP_HD void merge_move_old(const EditMerge &m, long long t)
{
    const int ra = m.inv[m.pa_old[t]], rb = m.inv[m.pb_old[t]], re = merge_min(ra, rb), rl = merge_max(ra, rb);
    const int i = m.oldpos[re];
    long long a = merge_cross_begin(m, i), b = merge_cross_end(m, i);
    const long long first = a;
    while (a < b) {      // cross pairs of box i whose later box ranks below rl
        const long long mid = a + ((b - a) >> 1);
        if (m.rank_l[mid] < rl) a = mid + 1;
        else b = mid;
    }
    const long long dst = m.offset[re] + (t - m.offset_old[i]) + (a - first);
    m.pa[dst] = m.pa_old[t]; m.pb[dst] = m.pb_old[t]; m.flag[dst] = m.flag_old[t]; m.st[dst] = m.st_old[t];
}
// thread x of T_new: cross pair x to its place
GCS_SWEEP_HD void merge_move_new(const EditMerge &m, long long x)
{
    const int re = m.rank_e[x], rl = m.rank_l[x], holder = m.oldpos[re];
    long long dst = m.offset[re] + (x - merge_cross_begin(m, holder));
    if (holder >= 0) {   // resident pairs of box `holder` whose later box ranks below rl
        long long a = m.offset_old[holder], b = a + m.count_old[holder];
        const long long first = a;
        while (a < b) {
            const long long mid = a + ((b - a) >> 1);
            if (merge_max(m.inv[m.pa_old[mid]], m.inv[m.pb_old[mid]]) < rl) a = mid + 1;
            else b = mid;
        }
        dst += a - first;
    }
    m.pa[dst] = m.pa_new[x]; m.pb[dst] = m.pb_new[x]; m.flag[dst] = m.flag_new[x]; m.st[dst] = m.st_new[x];
}

// ---- removal ----
struct EditRemove {
    int P;
    const int *newidx;              // [P] new index of a region that stays, -1 of one that goes
    const int *order, *count_old;   // the old sweep order and its segments
    const long long *offset_old;
    const int *pa_old, *pb_old, *st_old;
    const unsigned char *flag_old;
    int *kept;                      // [P] pairs of position i that stay
    const long long *dst;           // [P] where the pairs of position i go
    int *pa, *pb, *st;
    unsigned char *flag;
};
// thread i of P.  FILL = false: kept[i]; FILL = true: the pairs that stay, renumbered, from dst[i] on in their old order
template <bool FILL> GCS_SWEEP_HD void remove_segment(const EditRemove &e, int i)
{
    int total = 0;
    if (e.newidx[e.order[i]] >= 0) {
        long long at = FILL ? e.dst[i] : 0;
        const long long first = e.offset_old[i], last = first + e.count_old[i];
        for (long long t = first; t < last; ++t) {
            const int a = e.newidx[e.pa_old[t]], b = e.newidx[e.pb_old[t]];
            if (a < 0 || b < 0) continue;
            if (FILL) { e.pa[at] = a; e.pb[at] = b; e.flag[at] = e.flag_old[t]; e.st[at] = e.st_old[t]; ++at; }
            ++total;
        }
    }
    if (!FILL) e.kept[i] = total;
}
// row p of a [P][width] array to row newidx[p]
template <class V> GCS_SWEEP_HD void remove_compact_row(const V *src, V *dst, const int *newidx, int width, int p)
{
    const int q = newidx[p];
    if (q < 0) return;
    for (int c = 0; c < width; ++c) dst[(size_t)q * width + c] = src[(size_t)p * width + c];
}
// the rows of polytope p to where new_ptr puts them
GCS_SWEEP_HD void remove_compact_poly(const int *ptr, const int *new_ptr, const int *newidx, int n, int p, const double *A, const double *b,
                                      const double *nrm, double *A2, double *b2, double *nrm2)
{
    const int q = newidx[p];
    if (q < 0) return;
    const int rows = ptr[p + 1] - ptr[p];
    for (int r = 0; r < rows; ++r) {
        const size_t s = (size_t)ptr[p] + r, d = (size_t)new_ptr[q] + r;
        for (int c = 0; c < n; ++c) A2[d * n + c] = A[s * n + c];
        b2[d] = b[s];
        nrm2[d] = nrm[s];
    }
}

// ---- host side ----
// the keep mask as new indices: newidx[p] = p minus the removed regions below it, -1 for a removed one.  false: an index out of range
// or given twice (newidx is then unspecified).  Returns the number that stay through *left.
inline bool remove_renumber(int P, int num_removed, const int *regions, int *newidx, int *left)
{
    for (int p = 0; p < P; ++p) newidx[p] = 0;
    for (int r = 0; r < num_removed; ++r) {
        if (regions[r] < 0 || regions[r] >= P || newidx[regions[r]] < 0) return false;
        newidx[regions[r]] = -1;
    }
    int s = 0;
    for (int p = 0; p < P; ++p)
        if (newidx[p] == 0) newidx[p] = s++;
    *left = s;
    return true;
}

// exclusive scan of counts in 64 bits with the total behind it: offset[cells + 1].  false: the total is more than a pair list holds
inline bool edit_scan(const int *count, long long cells, long long *offset)
{
    long long s = 0;
    for (long long c = 0; c < cells; ++c) {
        offset[c] = s;
        s += count[c];
    }
    offset[cells] = s;
    return s <= (long long)INT32_MAX;
}

} // namespace gcsadmm_lp
