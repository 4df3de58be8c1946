// Host build of the scene edits of csrc/polytope_lp.hip (scene_edit_core.h): the steps of gcsadmm_scene_add_regions and
// gcsadmm_scene_remove_regions on the boxes and the pair list alone (no LPs), with the threads of a launch run one after the other and
// the ballot of cross_kernel formed from the 64 results of its lanes.  Test infrastructure: never shipped, never timed.
#include <vector>
#include "scene_edit_core.h"
using namespace gcsadmm_lp;

namespace {

// what a decided scene keeps of its sweep: order, sorted boxes, and the segments of the pair list (sweep_kernel's count pass)
template <int N> struct Resident {
    std::vector<int> order, count;
    std::vector<long long> offset;
    std::vector<double> slo, shi;
    long long total = 0;
    SortedBoxes boxes(int P) const { return SortedBoxes{P, slo.data(), shi.data(), order.data()}; }
    void sort(int P, const double *lo, const double *hi)
    {
        std::vector<double> lo0((size_t)P);
        order.resize((size_t)P); slo.resize((size_t)P * N + 1); shi.resize((size_t)P * N + 1);
        for (int p = 0; p < P; ++p) lo0[p] = lo[(size_t)p * N];
        sweep_order(lo0.data(), P, order.data());
        for (int t = 0; t < P; ++t) sweep_gather(lo, hi, order.data(), N, P, t, slo.data(), shi.data());
    }
    void sweep(int P, double pad)
    {
        count.assign((size_t)P, 0); offset.assign((size_t)P, 0);
        const SortedBoxes B = boxes(P);
        for (int k = 0; k < P; ++k) {
            SweepBox<N> bk;
            sweep_load_box<N>(B, k, pad, bk);
            const int end = sweep_window_end(B.lo, P, bk.hip[0]);
            for (int j = k + 1; j < end; ++j) count[k] += sweep_test<N>(B, bk, j, pad) ? 1 : 0;
        }
        sweep_scan(count.data(), P, offset.data(), &total);
    }
};

// cross_kernel<N, FILL> over its whole grid
template <int N, bool FILL> void cross(const CrossSide &c, int sweepers, double pad)
{
    for (int k = 0; k < sweepers; ++k)
        for (long long chunk = 0; chunk < c.chunks; ++chunk) {
            SweepBox<N> bk;
            sweep_load_box<N>(c.S, k, pad, bk);
            int w0, w1;
            cross_window<N>(c, k, bk, w0, w1);
            const size_t cell = (size_t)(c.cell0 + (long long)k * c.chunks + chunk);
            int total = 0;
            if (cross_chunk_live(chunk, w0, w1)) {
                const int re = cross_sweeper_rank(c, k, w0);
                long long pos = FILL ? c.offset[cell] : 0;
                for (int stride = 0; stride < EDIT_CHUNK / SWEEP_WAVE; ++stride) {
                    bool hit[SWEEP_WAVE];
                    int j[SWEEP_WAVE];
                    unsigned long long mask = 0;
                    for (int lane = 0; lane < SWEEP_WAVE; ++lane) {
                        hit[lane] = cross_hit<N>(c, bk, w0, w1, chunk, stride, lane, pad, j[lane]);
                        if (hit[lane]) mask |= 1ull << lane;
                    }
                    if (FILL) {
                        for (int lane = 0; lane < SWEEP_WAVE; ++lane)
                            if (hit[lane]) cross_store(c, pos + sweep_rank(mask, lane), re, j[lane]);
                        pos += sweep_hits(mask);
                    } else {
                        total += sweep_hits(mask);
                    }
                }
            }
            if (!FILL) c.count[cell] = total;
        }
}

template <int N>
long long add(int P, int K, const double *lo, const double *hi, double pad, long long T_old, const int *pa, const int *pb,
              const unsigned char *flag, const int *st, int *opa, int *opb, unsigned char *oflag, int *ost, long long capacity, long long *num_new)
{
    const int PK = P + K;
    Resident<N> old, app, all;
    old.sort(P, lo, hi);
    old.sweep(P, pad);
    if (old.total != T_old) return -2;      // the list handed in is not the resident boxes' list
    app.sort(K, lo + (size_t)P * N, hi + (size_t)P * N);
    std::vector<int> arank((size_t)K + 1), inv((size_t)PK + 1), oldpos((size_t)PK + 1);
    all.order.resize((size_t)PK + 1);
    const EditRanks ranks{P, K, old.slo.data(), app.slo.data(), old.order.data(), app.order.data(), arank.data(), all.order.data(),
                          inv.data(), oldpos.data()};
    for (int t = 0; t < PK; ++t) edit_rank(ranks, t);
    all.slo.resize((size_t)PK * N + 1); all.shi.resize((size_t)PK * N + 1);
    for (int t = 0; t < PK; ++t) sweep_gather(lo, hi, all.order.data(), N, PK, t, all.slo.data(), all.shi.data());

    CrossSide F{}, B{};
    F.S = app.boxes(K); F.T = all.boxes(PK); F.srank = arank.data(); F.chunks = edit_chunks(PK); F.cell0 = 0;
    B.S = old.boxes(P); B.T = F.S; B.trank = arank.data(); B.chunks = edit_chunks(K); B.cell0 = (long long)K * F.chunks;
    F.norder = B.norder = all.order.data();
    const long long cells = B.cell0 + (long long)P * B.chunks;
    std::vector<int> cell_count((size_t)cells + 1);
    std::vector<long long> cell_off((size_t)cells + 1);
    F.count = B.count = cell_count.data();
    cross<N, false>(F, K, pad); cross<N, false>(B, P, pad);
    if (!edit_scan(cell_count.data(), cells, cell_off.data())) return -1;
    const long long Tn = cell_off[(size_t)cells], T = T_old + Tn;
    *num_new = Tn;
    if (T > capacity) return T;
    std::vector<int> rank_e((size_t)Tn + 1), rank_l((size_t)Tn + 1), npa((size_t)Tn + 1), npb((size_t)Tn + 1), nst((size_t)Tn + 1, -9);
    std::vector<unsigned char> nflag((size_t)Tn + 1, 255);      // undecided until their LPs have run
    F.offset = B.offset = cell_off.data(); F.limit = B.limit = Tn;
    F.rank_e = B.rank_e = rank_e.data(); F.rank_l = B.rank_l = rank_l.data(); F.pair_a = B.pair_a = npa.data(); F.pair_b = B.pair_b = npb.data();
    cross<N, true>(F, K, pad); cross<N, true>(B, P, pad);

    EditMerge m{};
    m.P = P; m.K = K; m.T_old = T_old; m.T_new = Tn; m.chunks_f = F.chunks; m.chunks_b = B.chunks; m.cell_off = cell_off.data();
    m.oldpos = oldpos.data(); m.inv = inv.data(); m.count_old = old.count.data(); m.offset_old = old.offset.data();
    m.pa_old = pa; m.pb_old = pb; m.st_old = st; m.flag_old = flag;
    m.rank_e = rank_e.data(); m.rank_l = rank_l.data(); m.pa_new = npa.data(); m.pb_new = npb.data(); m.st_new = nst.data(); m.flag_new = nflag.data();
    std::vector<int> count((size_t)PK + 1);
    std::vector<long long> offset((size_t)PK + 1);
    m.count = count.data();
    for (int r = 0; r < PK; ++r) merge_count(m, r);
    long long total = 0;
    if (!sweep_scan(count.data(), PK, offset.data(), &total) || total != T) return -3;
    m.offset = offset.data(); m.pa = opa; m.pb = opb; m.st = ost; m.flag = oflag;
    for (long long t = 0; t < T_old; ++t) merge_move_old(m, t);
    for (long long x = 0; x < Tn; ++x) merge_move_new(m, x);
    return T;
}

template <int N>
long long remove(int P, const double *lo, const double *hi, double pad, int R, const int *regions, long long T_old, const int *pa, const int *pb,
                 const unsigned char *flag, const int *st, int *newidx, int *opa, int *opb, unsigned char *oflag, int *ost)
{
    int left = 0;
    if (!remove_renumber(P, R, regions, newidx, &left)) return -1;
    Resident<N> old;
    old.sort(P, lo, hi);
    old.sweep(P, pad);
    if (old.total != T_old) return -2;
    std::vector<int> kept((size_t)P + 1);
    std::vector<long long> dst((size_t)P + 1);
    EditRemove e{};
    e.P = P; e.newidx = newidx; e.order = old.order.data(); e.count_old = old.count.data(); e.offset_old = old.offset.data();
    e.pa_old = pa; e.pb_old = pb; e.st_old = st; e.flag_old = flag; e.kept = kept.data();
    for (int i = 0; i < P; ++i) remove_segment<false>(e, i);
    long long T = 0;
    for (int i = 0; i < P; ++i) { dst[i] = T; T += kept[i]; }
    e.dst = dst.data(); e.pa = opa; e.pb = opb; e.st = ost; e.flag = oflag;
    for (int i = 0; i < P; ++i) remove_segment<true>(e, i);
    return T;
}

} // namespace

// call<n> args for n = 1 .. 8 (-99: not dispatched)
#define EDIT_DIMS(call, args)                                                                                            \
    switch (n) {                                                                                                         \
    case 1: return call<1> args; case 2: return call<2> args; case 3: return call<3> args; case 4: return call<4> args;  \
    case 5: return call<5> args; case 6: return call<6> args; case 7: return call<7> args; case 8: return call<8> args;  \
    }                                                                                                                    \
    return -99

// The pair list (with flags and statuses) of the resident boxes lo[0 .. P) after boxes lo[P .. P + K) are added: returns its length
// (-1: too many pairs; -2: the list handed in is not the resident boxes'), fills the outputs when they have room (capacity entries each);
// the new pairs carry flag 255 and status -9.  *num_new: the number of new pairs.
extern "C" long long edit_emu_add(int n, int P, int K, const double *lo, const double *hi, double pad, long long T_old, const int *pa, const int *pb,
                                  const unsigned char *flag, const int *st, int *opa, int *opb, unsigned char *oflag, int *ost, long long capacity,
                                  long long *num_new)
{
    EDIT_DIMS(add, (P, K, lo, hi, pad, T_old, pa, pb, flag, st, opa, opb, oflag, ost, capacity, num_new));
}

// The same list after regions[0 .. R) are removed from the P boxes: returns its length (-1: an index out of range or given twice; -2: as
// above), fills newidx[P] (new index, -1 for a removed region) and the outputs (room for T_old entries each).
extern "C" long long edit_emu_remove(int n, int P, const double *lo, const double *hi, double pad, int R, const int *regions, long long T_old,
                                     const int *pa, const int *pb, const unsigned char *flag, const int *st, int *newidx, int *opa, int *opb,
                                     unsigned char *oflag, int *ost)
{
    EDIT_DIMS(remove, (P, lo, hi, pad, R, regions, T_old, pa, pb, flag, st, newidx, opa, opb, oflag, ost));
}

// edit_scan as the library calls it: 1 if a pair list can hold the total, 0 if not; offset[cells + 1]
extern "C" int edit_emu_scan(const int *count, long long cells, long long *offset) { return edit_scan(count, cells, offset) ? 1 : 0; }
