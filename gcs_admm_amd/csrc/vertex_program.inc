// vertex_program.h -- the per-wavefront program of the x-update (vertex step) kernel.
//
// One 64-lane wavefront (= one workgroup) solves several vertex sub-problems at once.
// A vertex with d incident edges occupies d+1 consecutive lanes ("group"):
//     lane 0 of the group  = the BORDER lane: unknowns (z_v, y_v) with facet rows 1,2
//                            (reference admm_solver_v3.py:420-426), the cone t >= |z_v1 - z_v2|
//                            (:380-384), x_v, and all group-level linear algebra;
//     lanes 1..d           = one BLOCK lane per incident edge: unknowns (O_e, y_e) with facet
//                            rows 3,4 (:434-440) and the consensus penalty (:392-413).
// Groups are placed in the wavefront by group_base(): back to back, or moved up so that no side segment of a
// group straddles a 16-lane row (the segmented reductions then use DPP row shifts).
// Rows 1,2 have exactly the shape of rows 3,4 with (z_v, y_v) in place of (O_e, y_e), so border
// and block lanes run the same row passes in lock step.  Constraints 5-7 (:443-464) are the
// reductions of SURVEY.md Appendix A.3 plus the two flow equalities, eliminated through the
// per-side sums B_in / B_out (see DESIGN.md section 4).
//
// The program is written as barrier-separated PHASES over a per-lane state struct, so that the
// same code runs as a HIP kernel (state in registers, LDS = __shared__) and, for debugging on a
// machine without a GPU, as a lock-step host emulation (tests/hostemu, never shipped or timed).
#include <math.h>
#include <stdint.h>

#include "step_args.h"
#include "warm_start.h"

// diagnostic builds (-DGCS_DUP=k): part k of the border factorisation is executed twice; the kernel time added
// is the cost of that part in place (tools/variant_time.py)
#ifndef GCS_DUP
#define GCS_DUP 0
#endif
#define GCS_REPEAT(k) for (int rep_ = 0; rep_ < (GCS_DUP == (k) ? 2 : 1); ++rep_)
#if GCS_DUP && defined(__HIP_DEVICE_COMPILE__)
#define GCS_REPEAT_FENCE() asm volatile("" ::: "memory")
#else
#define GCS_REPEAT_FENCE()
#endif
// GCS_STAMP marks the section boundaries of the border-lane code.  In the product build it is a compiler-level
// memory fence: with every slot array at a constant offset the optimiser would otherwise forward stored values
// to later loads and hoist loads across whole phases, and the longer live ranges spill (0 -> ~550 B/lane scratch).
#if !defined(GCS_STAMP) && defined(__HIP_DEVICE_COMPILE__)
#ifndef GCS_NOFENCE
#define GCS_NOFENCE 0      // diagnostic: bit k set = section boundary k is not fenced
#endif
#define GCS_STAMP(k) do { if (!((GCS_NOFENCE >> (k)) & 1)) asm volatile("" ::: "memory"); } while (0)
#endif
#ifndef GCS_STAMP
#define GCS_STAMP(k)
#endif
namespace GCS_NS {

// GCS_BOX: every polytope is an axis-aligned box with its facets in the canonical order [+e_0 .. +e_{N-1}, -e_0 .. -e_{N-1}]
// (the lattice configurations): a facet normal has one entry +-1, and the facet-row passes drop the products with its zeros
// at compile time.  x * a_j[k] is written GCS_AMUL(x, k); for a zero entry it yields -0.0, which an addition drops when the
// loops are unrolled (x * 0.0 would not be dropped: it can be NaN).
#if GCS_BOX
template <int N> GCS_HD double amul(double x, int j, int k) { return (j < N ? j : j - N) != k ? -0.0 : (j < N ? x : -x); }
template <int N> GCS_HD double amul2(double x, int j, int k, int l) { const int kk = j < N ? j : j - N; return (kk == k && kk == l) ? x : -0.0; }
#define GCS_AMUL(x, k) amul<N>((x), j, (k))
#define GCS_AMUL2(x, k, l) amul2<N>((x), j, (k), (l))
#else
#define GCS_AMUL(x, k) ((x) * a[k])
#define GCS_AMUL2(x, k, l) ((x) * a[k] * a[l])
#endif

constexpr int WAVE = 64;
constexpr int FIXED_FACETS = GCS_MFIX;   // 0: any facet count, facet-row duals in LDS; m: exactly m facets, duals in registers
constexpr int MAX_SLOTS = 7;     // vertices per wavefront

// the numerics shared with the workgroup program and the region terminals
using gcs_math::REG_DELTA;
using gcs_math::rcp;
using gcs_math::rcp1;
using gcs_math::rsqrt_nr;
using gcs_math::sqrt_nr;
using gcs_math::soc_det;
using gcs_math::soc_interior;
using gcs_math::soc_max_step;

GCS_HD constexpr int PK(int i, int j) { return i >= j ? i * (i + 1) / 2 + j : j * (j + 1) / 2 + i; }

template <int N> struct Dim {
    static constexpr int N2 = 2 * N, NW = 2 * N + 1, NB = 4 * N + 2, Q = N + 1;
    static constexpr int NB1 = NB - 1;   // border unknowns without the epigraph variable t (eliminated by hand)
    static constexpr int NS = N * (N + 1) / 2, NWS = NW * (NW + 1) / 2, NBS = NB1 * (NB1 + 1) / 2,
                         N2S = N2 * (N2 + 1) / 2;
    // reduction round 1 layout
    // three chunks, each computed right before it is staged:
    //   A: B_e, the block's unknowns, complementarity, X_ii   B: B_e X_e, B_e(-g)   C: X'BX, X'B(-g)
    static constexpr int R1_B = 0, R1_W = NWS, R1_GAP = R1_W + NW, R1_XII = R1_GAP + 1, R1A_N = R1_XII + 2 * NS,
                         R1_BX = R1A_N, R1_T = R1_BX + NW * N2, R1B_N = NW * N2 + NW,
                         R1_XBX = R1_T + NW, R1_XT = R1_XBX + N2S, R1C_N = N2S + N2, R1_N = R1_XT + N2;
    static constexpr int R2_BASE = R1_N, R2_N = 3;                 // amax (min), c1, c2
    static constexpr int R3_BASE = R2_BASE + R2_N;                 // corrector right-hand sides
    static constexpr int R3_T = 0, R3_XT = NW, R3_GX = NW + N2, R3_N = NW + 2 * N2;
    static constexpr int R4_BASE = R3_BASE + R3_N, R4_N = 1;       // amax (min)
    static constexpr int R0_BASE = R4_BASE + R4_N, R0_N = 1;       // scale (max), once before the loop
    static constexpr int NSUM = R0_BASE + R0_N;
};

// per-slot (vertex) LDS layout, in doubles.  Everything but the facet rows sits at a compile-time offset from
// the slot base (immediate ds offsets, and the compiler can tell the arrays apart); the facet rows, whose
// count is a run-time value in the generic program, come last.
template <int N> struct SlotLayout {
    using D = Dim<N>;
    int MM;
    static constexpr int CEN = 0;
    static constexpr int X = CEN + N;                 // x_v (centred), ping-pong by iteration parity
    static constexpr int NU = X + 2 * D::N2;          // multipliers of the two flow equalities
    static constexpr int DX = NU + 2 * D::NW;         // x part of the final Newton direction
    static constexpr int DXA = DX + D::N2;            // x part of the affine direction
    static constexpr int DNU = DXA + D::N2;
    static constexpr int SC = DNU + 2 * D::NW;        // scalars: 0 alpha, 1 sigma*mu, 2 done, 3 t, 4 soc_c0, 5 mu, 6 status,
                                                      // warm start (warm_start.h): 7 the solve restarts from the record, 8 mu_ref,
                                                      // 9 store the record now, 10 failed warm solve: start again cold, 11 first
                                                      // (re-centring) iteration of a warm solve, 12 iterations of the failed attempt, 13 rho, 14 dT (how far
                                                      // the targets moved since the record; < 0: no comparable record), 15 a warm attempt failed
    static constexpr int SIN = SC + 16;               // reduced sums over the incoming / outgoing block lanes
    static constexpr int SOUT = SIN + D::NSUM;
    static constexpr int BSI = SOUT + D::NSUM;        // inverse of B_in / B_out
    static constexpr int YS = BSI + 2 * D::NWS;       // Bs^{-1} BXs per side
    static constexpr int MF = YS + 2 * D::NW * D::N2; // Cholesky factor of the reduced border matrix
    // border-lane state (one lane per vertex touches it; in registers it would be charged to all 64 lanes)
    static constexpr int LSOC = MF + D::NBS;          // cone dual
    static constexpr int BX = LSOC + D::Q;            // x_v (current iterate)
    static constexpr int W = BX + D::N2;              // NT scaling, its inverse, W^{-2}
    static constexpr int WI = W + D::Q * D::Q;
    static constexpr int W2 = WI + D::Q * D::Q;
    static constexpr int LT = W2 + D::Q * D::Q;       // W lambda
    static constexpr int CV = LT + D::Q;
    static constexpr int DBA = CV + N;                // affine / final border directions
    static constexpr int DB = DBA + D::NB;
    static constexpr int DSSA = DB + D::NB;           // cone slack / dual directions
    static constexpr int DLSA = DSSA + D::Q;
    static constexpr int DSS = DLSA + D::Q;
    static constexpr int DLS = DSS + D::Q;
    static constexpr int KSOC = DLS + D::Q;
    static constexpr int FIXED = (KSOC + D::Q + 1) & ~1;
    int A, B, SIZE;
    GCS_HD explicit SlotLayout(int mm) : MM(mm)
    {
        A = FIXED;
        B = A + mm * N;
        SIZE = (B + mm + 1) & ~1;
        // LDS banks: the border lanes of a wavefront read the same offset of different slots in one instruction; with
        // a slot stride of 0 mod 64 dwords (m = 4: 832) they all hit one bank.  SIZE = 2 mod 4 doubles spreads up to
        // 16 slots over distinct banks (and keeps 16-byte alignment).
        if ((SIZE & 3) == 0) SIZE += 2;
    }
};

GCS_HD int lds_doubles(int n, int mm, int slots, int store_dl)
{
    // per-lane duals of rows a/b ( 2 halves x mm ), slots (the segmented reductions use wave shuffles, no staging)
    int per_lane = ((GCS_MFIX ? 2 : 4) + (store_dl ? 4 : 0)) * mm * WAVE;   // row duals: both kinds in LDS, or only the b-type ones when every polytope has GCS_MFIX facets
    int slot = n == 2 ? SlotLayout<2>(mm).SIZE : (n == 3 ? SlotLayout<3>(mm).SIZE : SlotLayout<6>(mm).SIZE);
    return per_lane + slots * slot;
}

// ---------------------------------------------------------------------------------------------
// small fixed-size dense helpers on packed lower-triangular storage (all indices compile-time)
// ---------------------------------------------------------------------------------------------
template <int NN> GCS_HD void chol_packed(double (&A)[NN * (NN + 1) / 2])
{
    double diag[NN];   // the pivot floor is relative to the original diagonal entry
#pragma unroll
    for (int j = 0; j < NN; ++j) diag[j] = A[PK(j, j)];
#pragma unroll
    for (int j = 0; j < NN; ++j) {
        double d = A[PK(j, j)];
#pragma unroll
        for (int k = 0; k < j; ++k) d -= A[PK(j, k)] * A[PK(j, k)];
        const double inv = rsqrt_nr(gcs_math::pivot_floor(d, diag[j]));
        A[PK(j, j)] = inv;          // the diagonal holds 1 / L_jj
#pragma unroll
        for (int i = j + 1; i < NN; ++i) {
            double s = A[PK(i, j)];
#pragma unroll
            for (int k = 0; k < j; ++k) s -= A[PK(i, k)] * A[PK(j, k)];
            A[PK(i, j)] = s * inv;
        }
    }
}
template <int NN> GCS_HD void chol_solve_packed(const double (&L)[NN * (NN + 1) / 2], double (&b)[NN])
{
#pragma unroll
    for (int i = 0; i < NN; ++i) {
        double s = b[i];
#pragma unroll
        for (int k = 0; k < i; ++k) s -= L[PK(i, k)] * b[k];
        b[i] = s * L[PK(i, i)];
    }
#pragma unroll
    for (int i = NN - 1; i >= 0; --i) {
        double s = b[i];
#pragma unroll
        for (int k = i + 1; k < NN; ++k) s -= L[PK(k, i)] * b[k];
        b[i] = s * L[PK(i, i)];
    }
}
// the same solve with the factor read from LDS
template <int NN> GCS_HD void chol_solve_lds(const double *L, double (&b)[NN])
{
#pragma unroll
    for (int i = 0; i < NN; ++i) {
        double s = b[i];
#pragma unroll
        for (int k = 0; k < i; ++k) s -= L[PK(i, k)] * b[k];
        b[i] = s * L[PK(i, i)];
    }
#pragma unroll
    for (int i = NN - 1; i >= 0; --i) {
        double s = b[i];
#pragma unroll
        for (int k = i + 1; k < NN; ++k) s -= L[PK(k, i)] * b[k];
        b[i] = s * L[PK(i, i)];
    }
}
template <int NN> GCS_HD void chol_inverse_packed(const double (&L)[NN * (NN + 1) / 2], double (&X)[NN * (NN + 1) / 2])
{
#pragma unroll
    for (int j = 0; j < NN; ++j) {
        double e[NN];
#pragma unroll
        for (int i = 0; i < NN; ++i) e[i] = (i == j) ? 1.0 : 0.0;
        chol_solve_packed<NN>(L, e);
#pragma unroll
        for (int i = j; i < NN; ++i) X[PK(i, j)] = e[i];
    }
}

// ---------------------------------------------------------------------------------------------
// second-order cone of dimension Q = N+1
// ---------------------------------------------------------------------------------------------
// Nesterov-Todd scaling W (symmetric, full QxQ): W lam = W^{-1} s.  Returns false on a boundary point.
template <int Q> GCS_HD bool soc_scaling(const double *s, const double *z, double *W, double *Wi, double *wb, double &eta)
{
    if (!gcs_math::soc_scaling_wb<Q>(s, z, wb, eta)) return false;
    const double ieta = rcp(eta), i1w0 = rcp(1.0 + wb[0]);
#pragma unroll
    for (int i = 0; i < Q; ++i)
#pragma unroll
        for (int j = 0; j < Q; ++j) {
            double w;
            if (i == 0 && j == 0) w = wb[0];
            else if (i == 0) w = wb[j];
            else if (j == 0) w = wb[i];
            else w = (i == j ? 1.0 : 0.0) + wb[i] * wb[j] * i1w0;
            W[i * Q + j] = eta * w;
            Wi[i * Q + j] = (((i == 0) != (j == 0)) ? -w : w) * ieta;
        }
    return true;
}

// ---------------------------------------------------------------------------------------------
// per-lane state
// ---------------------------------------------------------------------------------------------
enum Role : int { IDLE = 0, BORDER = 1, BLOCK = 2 };
enum LaneFlag : int { F_DONE = 1, F_STALLED = 2, F_FRESH = 4, F_SKIP = 8, F_SAVED = 16 };

template <int N> struct Lane {
    using D = Dim<N>;
    // identity
    int role, slot, d, d_in, glane, m;
    int out;                       // block lanes: 1 = outgoing.  (Vertex id, incidence slot and edge id are needed
                                   // at load and write-out only: recomputed there by lane_ids, not held in registers.)
    // unknowns of this lane: p = O_e (block) or z_v (border); yy = y_e or y_v
    double p[D::N2], yy;
    double dpa[D::NW], dp[D::NW];  // affine and final Newton directions of (p, yy)
    double T1[N], T2[N], Ty;       // block: targets (un-centred)
    // Hessian pieces of the rows owned by this lane (see pass_A)
    double K1[D::NS], K2[D::NS], k1y[N], k2y[N], kyy;
    double X1[D::NS], X2[D::NS], xy1[N], xy2[N];
    double P1[2 * D::N2 + 1], P2[2 * D::N2 + 1]; // G'(1/s) and G'(corr/s): parts p, y, x
    double g0[D::NW];              // gradient of the smooth objective part + equality multipliers
    double Bm[D::NWS];             // block: inverse of the block Hessian
    double gk[2 * D::N2 + 1];      // G' kappa
    double l5, l6;                 // duals of 0 <= y <= 1
#if GCS_MFIX
    double lamA[2 * GCS_MFIX];     // duals of the a-type facet rows in registers (fixed facet count); the b-type duals stay in LDS
#endif
    double amax, c1, c2, gap;
    // border lane only
    // (arrays live in the vertex's LDS slot: only one lane per vertex touches them, and keeping them
    //  in registers would charge every lane of the wavefront for them)
    // (border lane: t, soc_c0 (W^{-2} = [c0 cv'; cv C11], t eliminated by hand) and mu live in the slot scalars SC+3..5)
    int iters, status, bad;
    // one register for the lane's flags: F_DONE the vertex has stopped; F_STALLED vanishing step (border lane); F_FRESH the facet-row
    // and bound duals are still to be set from the slacks (first pass of a cold solve); F_SKIP the vertex starts again cold at the top
    // of the next iteration, sit this one out; F_SAVED (border lane) the record of this solve is written
    int fl;
    int segmask, seg_head, seg_steps;   // segmented reduction over the lanes of one side of a group (see seg_reduce)
    int seg_rowok;                      // the lane's side segment lies inside one 16-lane row (set-up only)
    double BX[D::NW * D::N2], t0[D::NW];   // block: B_e X_e and B_e(-g0), kept from chunk B to chunk C
    double scale0;
};

struct WaveShared {
    double *lamA, *lamB;   // [2*MM][64] duals of rows a (1 or 3) and b (2 or 4) (unused with a fixed facet count)
    double *dlA, *dlB;     // [2*MM][64] their final Newton directions (kernels built with SDL = 1 only): written by the
                           // step-bound pass, applied by the update pass, which then needs neither rows nor reciprocals
    double *slots;         // [MAX_SLOTS][slot size]
    int MM;
};

// the two duals of facet row (I, j) of this lane: registers when the facet count is fixed, else LDS
#if GCS_MFIX
#define GCS_DUAL_REFS(ra, rb) double &ra = L.lamA[I * GCS_MFIX + j]; double &rb = lb[(I * MM + j) * WAVE + lane]; (void)la
#else
#define GCS_DUAL_REFS(ra, rb) double &ra = la[(I * MM + j) * WAVE + lane]; double &rb = lb[(I * MM + j) * WAVE + lane]
#endif

// carve the wavefront's LDS allocation (lds_doubles) into the per-lane arrays and the vertex slots
GCS_HD void wave_shared_init(WaveShared &S, double *smem, int n, int mm, int store_dl)
{
    const int dual_rows = GCS_MFIX ? 0 : 2 * mm;      // a-type duals: registers when the facet count is fixed
    S.MM = mm;
    S.lamA = smem;
    S.lamB = S.lamA + dual_rows * WAVE;
    S.dlA = S.lamB + 2 * mm * WAVE;
    S.dlB = S.dlA + (store_dl ? 2 * mm * WAVE : 0);
    S.slots = S.dlB + (store_dl ? 2 * mm * WAVE : 0);
}

template <int N> GCS_HD double *slot_ptr(const WaveShared &S, const SlotLayout<N> &SL, int slot)
{
    return S.slots + (size_t)slot * SL.SIZE;
}

// ---------------------------------------------------------------------------------------------
// rows of one half i (compile-time) for a lane: F is called with (j, a[N], b, sa, sb, D? ...)
// sa = b*yy - a.p_i            (rows 1 / 3)
// sb = b*(1-yy) - a.(x_i - p_i) (rows 2 / 4)
// ---------------------------------------------------------------------------------------------
template <int N, int I, class F>
GCS_HD void rows_half(const Lane<N> &L, const double *A, const double *bc, const double *x, F &&f)
{
    double xi[N];   // loop invariant: read once (the stores of the passes could alias it for the compiler)
#pragma unroll
    for (int k = 0; k < N; ++k) xi[k] = x[I * N + k];
#if GCS_MFIX
#pragma unroll
    for (int j = 0; j < GCS_MFIX; ++j) {
#else
#pragma unroll 2
    for (int j = 0; j < L.m; ++j) {
#endif
        double a[N];
#pragma unroll
        for (int k = 0; k < N; ++k) a[k] = GCS_BOX ? 0.0 : A[j * N + k];     // (box: the normal is implied by j, never read)
        const double b = bc[j];
        double ap = 0, ax = 0;
#pragma unroll
        for (int k = 0; k < N; ++k) { ap += GCS_AMUL(L.p[I * N + k], k); ax += GCS_AMUL(xi[k], k); }
        const double sa = b * L.yy - ap;
        const double sb = b * (1.0 - L.yy) - (ax - ap);
        f(j, a, b, sa, sb);
    }
}

// direction slacks of one row: dsa = b*dy - a.dp_i ; dsb = -b*dy - a.(dx_i - dp_i)
template <int N, int I>
GCS_HD void row_dir(int j, const double (&a)[N], double b, const double (&dp)[2 * N + 1], const double *dx, double &dsa, double &dsb)
{
    (void)j;
    double adp = 0, adx = 0;
#pragma unroll
    for (int k = 0; k < N; ++k) { adp += GCS_AMUL(dp[I * N + k], k); adx += GCS_AMUL(dx[I * N + k], k); }
    dsa = b * dp[2 * N] - adp;
    dsb = -b * dp[2 * N] - (adx - adp);
}

// ---------------------------------------------------------------------------------------------
// PASS A: slacks, scalings, Hessian pieces, complementarity, G'lambda
// ---------------------------------------------------------------------------------------------
template <int N, int I>
GCS_HD void pass_A_half(Lane<N> &L, const double *A, const double *bc, const double *x, double *la, double *lb,
                        int MM, int lane, bool first, double (&Ki)[Dim<N>::NS], double (&kiy)[N],
                        double (&Xi)[Dim<N>::NS], double (&xyi)[N])
{
    rows_half<N, I>(L, A, bc, x, [&](int j, const double(&a)[N], double b, double sa, double sb) {
        GCS_DUAL_REFS(ra, rb);
        const double isa = rcp1(sa), isb = rcp1(sb);
        if (first) { ra = isa; rb = isb; }
        if (!(sa > 0.0) || !(sb > 0.0)) L.bad = 1;
        const double l_a = ra, l_b = rb;
        const double Da = l_a * isa, Db = l_b * isb, Ds = Da + Db;
#pragma unroll
        for (int k = 0; k < N; ++k) {
#pragma unroll
            for (int l = 0; l <= k; ++l) {
                Ki[PK(k, l)] += GCS_AMUL2(Ds, k, l);
                Xi[PK(k, l)] += GCS_AMUL2(Db, k, l);
            }
            kiy[k] += GCS_AMUL(-(Ds * b), k);
            xyi[k] += GCS_AMUL(Db * b, k);
        }
        L.kyy += Ds * b * b;
        L.gap += sa * l_a + sb * l_b;
    });
}

template <int N>
GCS_HD void pass_A(Lane<N> &L, const WaveShared &S, const SlotLayout<N> &SL, int lane, int par, double rho, double eps_edge)
{
    using D = Dim<N>;
    if (L.role == IDLE || (L.fl & F_DONE)) return;
    const bool first = (L.fl & F_FRESH) != 0;
    L.fl &= ~F_FRESH;
    double *sl = slot_ptr<N>(S, SL, L.slot);
    const double *A = sl + SL.A, *bc = sl + SL.B, *cen = sl + SL.CEN, *x = sl + SL.X + par * D::N2;
#pragma unroll
    for (int k = 0; k < D::NS; ++k) { L.K1[k] = L.K2[k] = L.X1[k] = L.X2[k] = 0; }
#pragma unroll
    for (int k = 0; k < N; ++k) { L.k1y[k] = L.k2y[k] = L.xy1[k] = L.xy2[k] = 0; }
    L.kyy = 0; L.gap = 0; L.bad = 0;
    pass_A_half<N, 0>(L, A, bc, x, S.lamA, S.lamB, S.MM, lane, first, L.K1, L.k1y, L.X1, L.xy1);
    pass_A_half<N, 1>(L, A, bc, x, S.lamA, S.lamB, S.MM, lane, first, L.K2, L.k2y, L.X2, L.xy2);
    // bounds 0 <= yy <= 1
    {
        const double s5 = L.yy, s6 = 1.0 - L.yy;
        const double is5 = rcp1(s5), is6 = rcp1(s6);
        if (first) { L.l5 = is5; L.l6 = is6; }
        L.kyy += L.l5 * is5 + L.l6 * is6;
        L.gap += s5 * L.l5 + s6 * L.l6;
        if (!(s5 > 0.0) || !(s6 > 0.0)) L.bad = 1;
    }
    if (L.bad) L.gap = 0.0 / 0.0;   // poisons mu: the border lane stops this vertex with status -3
#pragma unroll
    for (int k = 0; k < N; ++k) { L.K1[PK(k, k)] += REG_DELTA; L.K2[PK(k, k)] += REG_DELTA; }
    L.kyy += REG_DELTA;
    if (L.role == BLOCK) {
        const double *nu = sl + SL.NU + (L.out ? D::NW : 0);
        double gy = 0;
#pragma unroll
        for (int k = 0; k < N; ++k) {
            const double g1 = rho * (L.p[k] + L.yy * cen[k] - L.T1[k]);
            const double g2 = L.out ? rho * (L.p[N + k] + L.yy * cen[k] - L.T2[k]) : 0.0;
            L.g0[k] = g1 - nu[k] + REG_DELTA * L.p[k];
            L.g0[N + k] = g2 - nu[N + k] + REG_DELTA * L.p[N + k];
            gy += cen[k] * (g1 + g2);
            L.K1[PK(k, k)] += rho;
            L.k1y[k] += rho * cen[k];
            L.kyy += rho * cen[k] * cen[k];
            if (L.out) {
                L.K2[PK(k, k)] += rho;
                L.k2y[k] += rho * cen[k];
                L.kyy += rho * cen[k] * cen[k];
            }
        }
        L.g0[2 * N] = rho * (L.yy - L.Ty) + eps_edge + gy - nu[2 * N] + REG_DELTA * L.yy;
        L.kyy += rho;
    } else {
        const double *nu = sl + SL.NU;
#pragma unroll
        for (int k = 0; k < D::NW; ++k) L.g0[k] = nu[k] + nu[D::NW + k] + REG_DELTA * (k < D::N2 ? L.p[k] : L.yy);
    }
}

// block lanes: factor the arrow Hessian [K1 0 k1y; 0 K2 k2y; . . kyy], explicit inverse Bm,
// products with X = d(omega)/d(x) coupling, and stage round-1 values
template <int N> struct BlockProducts {
    using D = Dim<N>;
    double BX[D::NW * D::N2];
    double XBX[D::N2S];
};

template <int N> GCS_HD void block_factor(Lane<N> &L)
{
    using D = Dim<N>;
    // Cholesky of the 2n+1 arrow matrix in the variable order (O_1, O_2, y): identical pivots to
    // the dense factorisation of the oracle because O_1 and O_2 are not directly coupled.
    double F1[D::NS], F2[D::NS];
#pragma unroll
    for (int k = 0; k < D::NS; ++k) { F1[k] = L.K1[k]; F2[k] = L.K2[k]; }
    chol_packed<N>(F1);
    chol_packed<N>(F2);
    // l_i = L_i^{-1} k_iy  (forward substitution only)
    double l1[N], l2[N];
#pragma unroll
    for (int i = 0; i < N; ++i) {
        double s1 = L.k1y[i], s2 = L.k2y[i];
#pragma unroll
        for (int k = 0; k < i; ++k) { s1 -= F1[PK(i, k)] * l1[k]; s2 -= F2[PK(i, k)] * l2[k]; }
        l1[i] = s1 * F1[PK(i, i)];
        l2[i] = s2 * F2[PK(i, i)];
    }
    double dy = L.kyy;
#pragma unroll
    for (int k = 0; k < N; ++k) dy -= l1[k] * l1[k] + l2[k] * l2[k];
    const double isy = rcp(gcs_math::pivot_floor(dy, L.kyy));
    // u_i = K_i^{-1} k_iy = L_i^{-T} l_i
    double u1[N], u2[N];
#pragma unroll
    for (int i = N - 1; i >= 0; --i) {
        double s1 = l1[i], s2 = l2[i];
#pragma unroll
        for (int k = i + 1; k < N; ++k) { s1 -= F1[PK(k, i)] * u1[k]; s2 -= F2[PK(k, i)] * u2[k]; }
        u1[i] = s1 * F1[PK(i, i)];
        u2[i] = s2 * F2[PK(i, i)];
    }
    double I1[D::NS], I2[D::NS];
    chol_inverse_packed<N>(F1, I1);
    chol_inverse_packed<N>(F2, I2);
    // B = [I1 + u1 u1'/sy, u1 u2'/sy, -u1/sy; . , I2 + u2 u2'/sy, -u2/sy; . . 1/sy]
#pragma unroll
    for (int i = 0; i < N; ++i) {
#pragma unroll
        for (int j = 0; j <= i; ++j) {
            L.Bm[PK(i, j)] = I1[PK(i, j)] + u1[i] * u1[j] * isy;
            L.Bm[PK(N + i, N + j)] = I2[PK(i, j)] + u2[i] * u2[j] * isy;
        }
#pragma unroll
        for (int j = 0; j < N; ++j) L.Bm[PK(N + i, j)] = u2[i] * u1[j] * isy;
        L.Bm[PK(2 * N, i)] = -u1[i] * isy;
        L.Bm[PK(2 * N, N + i)] = -u2[i] * isy;
    }
    L.Bm[PK(2 * N, 2 * N)] = isy;
}

// y = Bm * r
template <int N> GCS_HD void block_apply(const Lane<N> &L, const double (&r)[2 * N + 1], double (&y)[2 * N + 1])
{
    constexpr int NW = 2 * N + 1;
#pragma unroll
    for (int i = 0; i < NW; ++i) {
        double s = 0;
#pragma unroll
        for (int k = 0; k < NW; ++k) s += L.Bm[PK(i, k)] * r[k];
        y[i] = s;
    }
}
// (X dx): X = [-X1 0; 0 -X2; xy1' xy2'] (rows O_1, O_2, y ; columns x_1, x_2)
template <int N> GCS_HD void X_apply(const Lane<N> &L, const double *dx, double (&y)[2 * N + 1])
{
    double sy = 0;
#pragma unroll
    for (int k = 0; k < N; ++k) {
        double s1 = 0, s2 = 0;
#pragma unroll
        for (int l = 0; l < N; ++l) { s1 -= L.X1[PK(k, l)] * dx[l]; s2 -= L.X2[PK(k, l)] * dx[N + l]; }
        y[k] = s1; y[N + k] = s2;
        sy += L.xy1[k] * dx[k] + L.xy2[k] * dx[N + k];
    }
    y[2 * N] = sy;
}
// X' t
template <int N> GCS_HD void XT_apply(const Lane<N> &L, const double (&t)[2 * N + 1], double (&y)[2 * N])
{
#pragma unroll
    for (int a = 0; a < N; ++a) {
        double s1 = L.xy1[a] * t[2 * N], s2 = L.xy2[a] * t[2 * N];
#pragma unroll
        for (int k = 0; k < N; ++k) { s1 -= L.X1[PK(a, k)] * t[k]; s2 -= L.X2[PK(a, k)] * t[N + k]; }
        y[a] = s1; y[N + a] = s2;
    }
}

// reduction round 1 of a block lane, produced chunk by chunk right before each chunk is reduced
template <int N> GCS_HD void block_chunk_A(Lane<N> &L, double (&v)[Dim<N>::R1A_N], bool active)
{
    using D = Dim<N>;
#pragma unroll
    for (int k = 0; k < D::R1A_N; ++k) v[k] = 0.0;
    if (!active) return;
    block_factor<N>(L);
#pragma unroll
    for (int k = 0; k < D::NWS; ++k) v[D::R1_B + k] = L.Bm[k];
#pragma unroll
    for (int k = 0; k < D::N2; ++k) v[D::R1_W + k] = L.p[k];
    v[D::R1_W + D::N2] = L.yy;
    v[D::R1_GAP] = L.gap;
#pragma unroll
    for (int k = 0; k < D::NS; ++k) {
        v[D::R1_XII + k] = L.X1[k];
        v[D::R1_XII + D::NS + k] = L.X2[k];
    }
}
template <int N> GCS_HD void block_chunk_B(Lane<N> &L, double (&v)[Dim<N>::R1B_N], bool active)
{
    using D = Dim<N>;
#pragma unroll
    for (int k = 0; k < D::R1B_N; ++k) v[k] = 0.0;
    if (!active) return;
    // BX columns: B * X e_c
#pragma unroll
    for (int c = 0; c < D::N2; ++c) {
        double col[D::NW], e[D::N2], bc_[D::NW];
#pragma unroll
        for (int k = 0; k < D::N2; ++k) e[k] = (k == c) ? 1.0 : 0.0;
        X_apply<N>(L, e, col);
        block_apply<N>(L, col, bc_);
#pragma unroll
        for (int i = 0; i < D::NW; ++i) { L.BX[i * D::N2 + c] = bc_[i]; v[i * D::N2 + c] = bc_[i]; }
    }
    double r[D::NW];
#pragma unroll
    for (int k = 0; k < D::NW; ++k) r[k] = -L.g0[k];
    block_apply<N>(L, r, L.t0);
#pragma unroll
    for (int k = 0; k < D::NW; ++k) v[D::NW * D::N2 + k] = L.t0[k];
}
template <int N> GCS_HD void block_chunk_C(Lane<N> &L, double (&v)[Dim<N>::R1C_N], bool active)
{
    using D = Dim<N>;
#pragma unroll
    for (int k = 0; k < D::R1C_N; ++k) v[k] = 0.0;
    if (!active) return;
    // XBX = X' (B X)
#pragma unroll
    for (int c = 0; c < D::N2; ++c) {
        double col[D::NW], xt[D::N2];
#pragma unroll
        for (int i = 0; i < D::NW; ++i) col[i] = L.BX[i * D::N2 + c];
        XT_apply<N>(L, col, xt);
#pragma unroll
        for (int a = c; a < D::N2; ++a) v[PK(a, c)] = xt[a];
    }
    double xt0[D::N2];
    XT_apply<N>(L, L.t0, xt0);
#pragma unroll
    for (int k = 0; k < D::N2; ++k) v[D::N2S + k] = xt0[k];
}

template <class T> struct VertexArgs;
template <int N, class T> GCS_HD double *warm_record(const Lane<N> &L, int wave, const VertexArgs<T> &a);

// ---------------------------------------------------------------------------------------------
// BORDER lane: convergence test, cone scaling, reduced border matrix, affine solve
// ---------------------------------------------------------------------------------------------
template <int N> struct BorderIdx {
    static constexpr int X1 = 0, X2 = N, Z1 = 2 * N, Z2 = 3 * N, YV = 4 * N, TT = 4 * N + 1;
};

// Newton solve with the stored factors.  gb: gradient (border, NB); t-sums and X't sums from LDS.
// SOLVE(r1) applies the factored reduced border matrix: from registers right after the factorisation
// (affine direction), from the copy in the LDS slot later (corrector).
template <int N, class SOLVE>
GCS_HD void border_solve(Lane<N> &L, double *sl, const SlotLayout<N> &SL, const double (&gb)[Dim<N>::NB],
                         const double *tin, const double *tout, const double *xtin, const double *xtout,
                         const double (&rp)[2][Dim<N>::NW], double *db, int dxoff, SOLVE &&solve)
{
    using D = Dim<N>;
    double rhs[D::NB];
#pragma unroll
    for (int k = 0; k < D::NB; ++k) rhs[k] = -gb[k];
#pragma unroll
    for (int c = 0; c < D::N2; ++c) rhs[c] -= xtin[c] + xtout[c];
    double u[2][D::NW];
#pragma unroll
    for (int s = 0; s < 2; ++s) {
        const double *Bsi = sl + SL.BSI + s * D::NWS;
        const double *BXs = sl + (s ? SL.SOUT : SL.SIN) + D::R1_BX;
        const double *ts = s ? tout : tin;
        double v[D::NW];
#pragma unroll
        for (int i = 0; i < D::NW; ++i) u[s][i] = rp[s][i] - ts[i];
#pragma unroll
        for (int i = 0; i < D::NW; ++i) {
            double a = 0;
#pragma unroll
            for (int k = 0; k < D::NW; ++k) a += Bsi[PK(i, k)] * u[s][k];
            v[i] = a;
        }
#pragma unroll
        for (int c = 0; c < D::N2; ++c) {
            double a = 0;
#pragma unroll
            for (int i = 0; i < D::NW; ++i) a += BXs[i * D::N2 + c] * v[i];
            rhs[c] -= a;
        }
#pragma unroll
        for (int i = 0; i < D::NW; ++i) rhs[D::N2 + i] -= v[i];
    }
    GCS_STAMP(8);
    {   // t eliminated: c0 dt + cv'(dz1 - dz2) = -gb[t]
        using BI = BorderIdx<N>;
        const double ic0 = rcp(sl[SlotLayout<N>::SC + 4]);
        const double gt = gb[BI::TT] * ic0;
        double r1[D::NB1];
#pragma unroll
        for (int k = 0; k < D::NB1; ++k) r1[k] = rhs[k];
#pragma unroll
        for (int k = 0; k < N; ++k) { r1[BI::Z1 + k] += (sl + SlotLayout<N>::CV)[k] * gt; r1[BI::Z2 + k] -= (sl + SlotLayout<N>::CV)[k] * gt; }
#pragma unroll
        for (int k = 0; k < N; ++k) r1[BI::Z2 + k] += r1[BI::Z1 + k];   // rhs in the (u, z_2) variables
        solve(r1);
#pragma unroll
        for (int k = 0; k < N; ++k) r1[BI::Z1 + k] += r1[BI::Z2 + k];   // dz_1 = du + dz_2
#pragma unroll
        for (int k = 0; k < D::NB1; ++k) db[k] = r1[k];
        double a = -gb[BI::TT];
#pragma unroll
        for (int k = 0; k < N; ++k) a -= (sl + SlotLayout<N>::CV)[k] * (db[BI::Z1 + k] - db[BI::Z2 + k]);
        db[BI::TT] = a * ic0;
    }
    GCS_STAMP(9);
#pragma unroll
    for (int s = 0; s < 2; ++s) {
        const double *Bsi = sl + SL.BSI + s * D::NWS;
        const double *BXs = sl + (s ? SL.SOUT : SL.SIN) + D::R1_BX;
        double w[D::NW];
#pragma unroll
        for (int i = 0; i < D::NW; ++i) {
            double a = db[D::N2 + i] + u[s][i];
#pragma unroll
            for (int c = 0; c < D::N2; ++c) a += BXs[i * D::N2 + c] * db[c];
            w[i] = a;
        }
#pragma unroll
        for (int i = 0; i < D::NW; ++i) {
            double a = 0;
#pragma unroll
            for (int k = 0; k < D::NW; ++k) a += Bsi[PK(i, k)] * w[k];
            sl[SL.DNU + s * D::NW + i] = a;
        }
    }
#pragma unroll
    for (int c = 0; c < D::N2; ++c) sl[dxoff + c] = db[c];
}

template <int N, class T>
GCS_HD void border_factor_and_affine(Lane<N> &L, const WaveShared &S, const SlotLayout<N> &SL, double ipm_tol, int max_iter, int wave,
                                     const VertexArgs<T> &a)
{
    using D = Dim<N>; using BI = BorderIdx<N>;
    if (L.role != BORDER || (L.fl & F_DONE)) return;
    double *sl = slot_ptr<N>(S, SL, L.slot);
    // warm start (warm_start.h).  The first iteration of a solve that restarts from the vertex's record is the re-centring Newton
    // step: no stop test, target mu_ref, no second-order term (flag SC + 11 for the lanes).  (The record's address is formed where
    // it is needed -- once per solve -- not held in registers across the factorisation.)
    const bool warm = sl[SL.SC + 7] != 0.0, first_warm = warm && L.iters == 0;
    sl[SL.SC + 11] = first_warm ? 1.0 : 0.0;
    const double *sin = sl + SL.SIN, *sout = sl + SL.SOUT;
    const int deg = (4 * L.m + 2) * (L.d + 1) + 1;
    // ---- complementarity and residuals ----
    double ssoc[D::Q];
    ssoc[0] = sl[SlotLayout<N>::SC + 3];
#pragma unroll
    for (int k = 0; k < N; ++k) ssoc[1 + k] = L.p[k] - L.p[N + k];
    double gap = L.gap + sin[D::R1_GAP] + sout[D::R1_GAP];
#pragma unroll
    for (int k = 0; k < D::Q; ++k) gap += ssoc[k] * (sl + SlotLayout<N>::LSOC)[k];
    const double mu = gap * rcp((double)deg);
    sl[SlotLayout<N>::SC + 5] = mu;
    double rp[2][D::NW];
    double rpmax = 0;
#pragma unroll
    for (int k = 0; k < D::NW; ++k) {
        const double zeta = (k < D::N2) ? L.p[k] : L.yy;
        rp[0][k] = zeta - sin[D::R1_W + k];
        rp[1][k] = zeta - sout[D::R1_W + k];
        rpmax = fmax(rpmax, fmax(fabs(rp[0][k]), fabs(rp[1][k])));
    }
    // stop on the barrier parameter alone (see oracle/gcs_oracle.c): insensitive to solve round-off
    (void)rpmax;
    // a vanishing step (stalled) means the linear algebra has run out of precision: accept the point if
    // the barrier parameter is within 1e3 of the target
    // the record the next solve of this vertex restarts from: the first iterate, after a step, at mu <= WS_SAVE mu_ref; every lane
    // of the group stores its part at the head of pass_B (flag SC + 9)
    sl[SL.SC + 9] = 0.0;
    if (a.warm != nullptr && !(L.fl & F_SAVED) && L.iters >= 1 && mu <= gcs_ws::WS_SAVE * sl[SL.SC + 8]) { L.fl |= F_SAVED; sl[SL.SC + 9] = 1.0; }
    // (gcs_math::mu_converged spelled out: the call changes the generated code here)
    const bool conv = !first_warm && (mu <= ipm_tol || ((L.fl & F_STALLED) && mu <= 1e3 * ipm_tol));
    bool stop = conv;
    // (a WARM solve does not leave through the precision-exhausted rule: it is repeated cold -- oracle/gcs_oracle.c)
    int status = conv ? ((warm && !(mu <= ipm_tol)) ? -7 : 0) : -1;
    if (!(mu > 0.0)) { stop = true; status = -3; }   // a slack left the cone (NaN from pass_A)
    if (!stop && L.iters >= max_iter) { stop = true; status = -1; }
    GCS_STAMP(0);
    // ---- cone scaling ----
    double wb[D::Q], eta = 1.0;
#pragma unroll
    for (int k = 0; k < D::Q; ++k) wb[k] = 0.0;
    GCS_REPEAT(1) if (!stop) {
        GCS_REPEAT_FENCE();
        if (!soc_scaling<D::Q>(ssoc, (sl + SlotLayout<N>::LSOC), (sl + SlotLayout<N>::W), (sl + SlotLayout<N>::WI), wb, eta)) { stop = true; status = gcs_math::boundary_status(mu, ipm_tol, warm); }
    }
    if (stop) {
        if (status != 0 && a.warm != nullptr) warm_record<N, T>(L, wave, a)[0] = 0.0;      // no restart from a solve that failed
        if (status != 0 && warm) {      // a failed warm solve is repeated cold: the group sits this iteration out (flag SC + 10)
            sl[SL.SC + 10] = 1.0; sl[SL.SC + 9] = 0.0;
            sl[SL.SC + 7] = 0.0; sl[SL.SC + 8] = gcs_ws::WS_COLD_REF;
            sl[SL.SC + 12] += (double)L.iters; sl[SL.SC + 15] = 1.0;
            L.fl |= F_SKIP;
            return;
        }
        L.fl |= F_DONE; L.status = status;
        sl[SL.SC + 2] = 1.0;
        sl[SL.SC + 6] = (double)status;   // read by every lane of the group at write-out
        return;
    }
    GCS_REPEAT(1)
#pragma unroll
    for (int i = 0; i < D::Q; ++i) {
        GCS_REPEAT_FENCE();
#pragma unroll
        for (int j = 0; j < D::Q; ++j) {
            double a = 0;
#pragma unroll
            for (int k = 0; k < D::Q; ++k) a += (sl + SlotLayout<N>::WI)[i * D::Q + k] * (sl + SlotLayout<N>::WI)[k * D::Q + j];
            (sl + SlotLayout<N>::W2)[i * D::Q + j] = a;
        }
        double a = 0;
#pragma unroll
        for (int k = 0; k < D::Q; ++k) a += (sl + SlotLayout<N>::W)[i * D::Q + k] * (sl + SlotLayout<N>::LSOC)[k];
        (sl + SlotLayout<N>::LT)[i] = a;
    }
    GCS_STAMP(1);
    // ---- reduced border matrix M (packed lower, order x1 x2 z1 z2 yv; in registers) ----
    // own rows of the border lane first, then side by side: factor B_s, invert, Y_s = Bs^{-1} BX_s, and the
    // side's terms go into M straight from registers (Bs^{-1} and Y_s are stored for the solves only)
    double M[D::NBS];
#pragma unroll
    for (int a = 0; a < D::N2; ++a)
#pragma unroll
        for (int c = 0; c <= a; ++c) {
            double v = (a == c ? REG_DELTA : 0.0);
            if (a < N && c < N) v += L.X1[PK(a, c)];
            if (a >= N && c >= N) v += L.X2[PK(a - N, c - N)];
            M[PK(a, c)] = v;
        }
#pragma unroll
    for (int i = 0; i < D::NW; ++i)
#pragma unroll
        for (int c = 0; c < D::N2; ++c) {
            double v = 0.0;
            if (i < N && c < N) v -= L.X1[PK(i, c)];
            if (i >= N && i < D::N2 && c >= N) v -= L.X2[PK(i - N, c - N)];
            if (i == D::N2) v += (c < N) ? L.xy1[c] : L.xy2[c - N];
            M[PK(D::N2 + i, c)] = v;
        }
#pragma unroll
    for (int i = 0; i < D::NW; ++i)
#pragma unroll
        for (int k = 0; k <= i; ++k) {
            double v = 0.0;
            if (i < N) v += L.K1[PK(i, k)];
            if (i >= N && i < D::N2 && k >= N) v += L.K2[PK(i - N, k - N)];
            if (i == D::N2) v += (k < N) ? L.k1y[k] : (k < D::N2 ? L.k2y[k - N] : L.kyy);
            M[PK(D::N2 + i, D::N2 + k)] = v;
        }
    GCS_REPEAT(2)
#pragma unroll
    for (int s = 0; s < 2; ++s) {
        GCS_STAMP(12);   // one side at a time: interleaving both doubles the temporaries
        const double *sum = s ? sout : sin;
        double Bsi[D::NWS];
        {
            double Bs[D::NWS];
#pragma unroll
            for (int k = 0; k < D::NWS; ++k) Bs[k] = sum[D::R1_B + k];
            chol_packed<D::NW>(Bs);
            chol_inverse_packed<D::NW>(Bs, Bsi);
        }
#pragma unroll
        for (int k = 0; k < D::NWS; ++k) sl[SL.BSI + s * D::NWS + k] = Bsi[k];
#pragma unroll
        for (int i = 0; i < D::NW; ++i)
#pragma unroll
            for (int k = 0; k <= i; ++k) M[PK(D::N2 + i, D::N2 + k)] += Bsi[PK(i, k)];       // zeta-zeta block
        GCS_STAMP(13);
        const double *bx = sum + D::R1_BX;   // read where used: 20 more live values would spill
#pragma unroll
        for (int c = 0; c < D::N2; ++c) {           // column c of Y_s, used at once
            double y[D::NW];
#pragma unroll
            for (int i = 0; i < D::NW; ++i) {
                double a = 0;
#pragma unroll
                for (int k = 0; k < D::NW; ++k) a += Bsi[PK(i, k)] * bx[k * D::N2 + c];
                y[i] = a;
                sl[SL.YS + s * D::NW * D::N2 + i * D::N2 + c] = a;
                M[PK(D::N2 + i, c)] += a;                                                    // zeta-x block
            }
#pragma unroll
            for (int a = c; a < D::N2; ++a) {       // x-x block: X_ii sums - X'BX sums + BX_s' Y_s
                double v = -sum[D::R1_XBX + PK(a, c)];
                if (a < N && c < N) v += sum[D::R1_XII + PK(a, c)];
                if (a >= N && c >= N) v += sum[D::R1_XII + D::NS + PK(a - N, c - N)];
#pragma unroll
                for (int k = 0; k < D::NW; ++k) v += bx[k * D::N2 + a] * y[k];
                M[PK(a, c)] += v;
            }
        }
    }
    GCS_STAMP(2);
    // Cone block.  With W^{-2} = eta^{-2}(2 v v' - J), v = (wb0, -wb1), eliminating t first leaves on
    // u = z_1 - z_2 the Schur complement Su = eta^{-2}(I - 2 wb1 wb1'/(2 wb0^2 - 1)), formed from this
    // closed form: a numerical pivot on t cancels catastrophically once the cone is active.
    double Su[N * N];
    {
        const double ie2 = rcp(eta * eta), g2 = 2.0 * rcp(2.0 * wb[0] * wb[0] - 1.0);
        sl[SlotLayout<N>::SC + 4] = ie2 * (2.0 * wb[0] * wb[0] - 1.0);
#pragma unroll
        for (int k = 0; k < N; ++k) {
            (sl + SlotLayout<N>::CV)[k] = -ie2 * 2.0 * wb[0] * wb[1 + k];
#pragma unroll
            for (int l = 0; l < N; ++l) Su[k * N + l] = ie2 * ((k == l ? 1.0 : 0.0) - g2 * wb[1 + k] * wb[1 + l]);
        }
    }
    GCS_STAMP(4);
    // Change of variables (u, z_2) = (z_1 - z_2, z_2): the cone term then sits on u alone.  In (z_1, z_2)
    // it enters as [Su -Su; -Su Su] and, with the cone inactive (t -> 0), Su grows like 1/mu, so that
    // eliminating z_1 before z_2 would cancel K_2 + Su - Su (K_1 + Su)^{-1} Su.
    {   // in place: first the (z2', z2') block, which needs the untouched cross entries, then the rest
#pragma unroll
        for (int k = 0; k < N; ++k)
#pragma unroll
            for (int l = 0; l <= k; ++l)
                M[PK(BI::Z2 + k, BI::Z2 + l)] += M[PK(BI::Z1 + k, BI::Z2 + l)] + M[PK(BI::Z2 + k, BI::Z1 + l)] + M[PK(BI::Z1 + k, BI::Z1 + l)];
#pragma unroll
        for (int i = 0; i < D::NB1; ++i) {
            if (i >= BI::Z2 && i < BI::Z2 + N) continue;
#pragma unroll
            for (int k = 0; k < N; ++k) M[PK(i, BI::Z2 + k)] += M[PK(i, BI::Z1 + k)];
        }
#pragma unroll
        for (int k = 0; k < N; ++k)
#pragma unroll
            for (int l = 0; l <= k; ++l) M[PK(BI::Z1 + k, BI::Z1 + l)] += Su[k * N + l];
        GCS_STAMP(5);
        chol_packed<D::NB1>(M);
        GCS_STAMP(6);
        GCS_REPEAT(5) {
            GCS_REPEAT_FENCE();
#pragma unroll
            for (int k = 0; k < D::NBS; ++k) sl[SL.MF + k] = M[k];
        }
#if GCS_DUP == 4 || GCS_DUP == 40
        GCS_REPEAT_FENCE();
#if GCS_DUP == 4
        chol_packed<D::NB1>(M);     // factor of the factor: garbage of the same cost, discarded by the reload
#endif
#pragma unroll
        for (int k = 0; k < D::NBS; ++k) M[k] = (M[k] == 1.25 ? 1.0 : 0.0) + sl[SL.MF + k];
#endif
    }
    GCS_STAMP(7);
    // ---- affine direction (kappa = 0) ----
    double gb[D::NB];
#pragma unroll
    for (int k = 0; k < D::N2; ++k) gb[k] = REG_DELTA * (sl + SlotLayout<N>::BX)[k];
#pragma unroll
    for (int k = 0; k < D::NW; ++k) gb[D::N2 + k] = L.g0[k];
    gb[BI::TT] = 1.0;
    GCS_REPEAT(6) {
    GCS_REPEAT_FENCE();
    border_solve<N>(L, sl, SL, gb, sin + D::R1_T, sout + D::R1_T, sin + D::R1_XT, sout + D::R1_XT, rp, (sl + SlotLayout<N>::DBA), SL.DXA,
                    [&](double (&r1)[D::NB1]) {
                        if constexpr (N == 2) chol_solve_packed<D::NB1>(M, r1);   // the factor is still in registers
                        else chol_solve_lds<D::NB1>(sl + SL.MF, r1);
                    });
    }
    GCS_STAMP(10);
}

// ---------------------------------------------------------------------------------------------
// direction of a lane's own unknowns from the border solution in LDS
// ---------------------------------------------------------------------------------------------
template <int N>
GCS_HD void lane_direction(Lane<N> &L, const double *sl, const SlotLayout<N> &SL, bool affine, double (&dp)[2 * N + 1])
{
    using D = Dim<N>;
    if (L.role == BLOCK) {
        const double *dnu = sl + SL.DNU + (L.out ? D::NW : 0);
        double xd[D::NW], r[D::NW];
        X_apply<N>(L, sl + (affine ? SL.DXA : SL.DX), xd);
#pragma unroll
        for (int k = 0; k < D::NW; ++k) r[k] = -(L.g0[k] + (affine ? 0.0 : L.gk[k])) + dnu[k] - xd[k];
        block_apply<N>(L, r, dp);
    } else {
        const double *db = affine ? (sl + SlotLayout<N>::DBA) : (sl + SlotLayout<N>::DB);
#pragma unroll
        for (int k = 0; k < D::NW; ++k) dp[k] = db[D::N2 + k];
    }
}

template <int N, class T>
GCS_HD void warm_store(Lane<N> &L, int lane, int wave, const VertexArgs<T> &a, const WaveShared &S, const SlotLayout<N> &SL);

// PASS B (after the affine solve): step bound, mu_aff sums, and the two vectors G'(1/s), G'(corr/s)
template <int N, int I>
GCS_HD void pass_B_half(Lane<N> &L, const double *A, const double *bc, const double *x, const double *dxa,
                        double *la, double *lb, int MM, int lane)
{
    rows_half<N, I>(L, A, bc, x, [&](int j, const double(&a)[N], double b, double sa, double sb) {
        GCS_DUAL_REFS(ra, rb);
        const double l_a = ra, l_b = rb;
        double dsa, dsb;
        row_dir<N, I>(j, a, b, L.dpa, dxa, dsa, dsb);
        const double ia = rcp1(sa), ib = rcp1(sb);
        const double qsa = dsa * ia, qsb = dsb * ib;                 // ds / s
        const double dla = -l_a - l_a * qsa, dlb = -l_b - l_b * qsb; // kappa = 0:  dl / l = -1 - ds / s
        // largest -ds/s and -dl/l over the rows; the step bound is its reciprocal
        L.amax = fmax(L.amax, fmax(fmax(-qsa, 1.0 + qsa), fmax(-qsb, 1.0 + qsb)));
        L.c1 += sa * dla + l_a * dsa + sb * dlb + l_b * dsb;
        L.c2 += dsa * dla + dsb * dlb;
        const double qa = dsa * dla * ia, qb = dsb * dlb * ib;
        // G rows: a-type (+a on p_i, -b on y), b-type (-a on p_i, +b on y, +a on x_i)
#pragma unroll
        for (int k = 0; k < N; ++k) {
            L.P1[I * N + k] += GCS_AMUL(ia - ib, k);
            L.P2[I * N + k] += GCS_AMUL(qa - qb, k);
            L.P1[2 * N + 1 + I * N + k] += GCS_AMUL(ib, k);
            L.P2[2 * N + 1 + I * N + k] += GCS_AMUL(qb, k);
        }
        L.P1[2 * N] += b * (ib - ia);
        L.P2[2 * N] += b * (qb - qa);
    });
}

template <int N, class T>
GCS_HD void pass_B(Lane<N> &L, const WaveShared &S, const SlotLayout<N> &SL, int lane, int par, int wave, const VertexArgs<T> &a)
{
    using D = Dim<N>;
    if (L.role == IDLE || (L.fl & F_DONE)) return;
    double *sl = slot_ptr<N>(S, SL, L.slot);
    if (sl[SL.SC + 10] != 0.0) { L.fl |= F_SKIP; return; }      // the vertex starts again cold at the top of the next iteration
    if (sl[SL.SC + 9] != 0.0) warm_store<N, T>(L, lane, wave, a, S, SL);
    if (sl[SL.SC + 2] != 0.0) { L.fl |= F_DONE; return; }
    lane_direction<N>(L, sl, SL, true, L.dpa);
    L.amax = 0.0; L.c1 = 0; L.c2 = 0;   // amax holds the largest ratio until the end of the pass
#pragma unroll
    for (int k = 0; k < 2 * D::N2 + 1; ++k) { L.P1[k] = 0; L.P2[k] = 0; }
    const double *dxa = sl + SL.DXA, *x = sl + SL.X + par * D::N2;
    pass_B_half<N, 0>(L, sl + SL.A, sl + SL.B, x, dxa, S.lamA, S.lamB, S.MM, lane);
    pass_B_half<N, 1>(L, sl + SL.A, sl + SL.B, x, dxa, S.lamA, S.lamB, S.MM, lane);
    {   // bounds: s5 = yy (G = -1), s6 = 1 - yy (G = +1)
        const double s5 = L.yy, s6 = 1.0 - L.yy, ds5 = L.dpa[2 * N], ds6 = -L.dpa[2 * N];
        const double i5 = rcp1(s5), i6 = rcp1(s6), q5 = ds5 * i5, q6 = ds6 * i6;
        const double dl5 = -L.l5 - L.l5 * q5, dl6 = -L.l6 - L.l6 * q6;
        L.amax = fmax(L.amax, fmax(fmax(-q5, 1.0 + q5), fmax(-q6, 1.0 + q6)));
        L.c1 += s5 * dl5 + L.l5 * ds5 + s6 * dl6 + L.l6 * ds6;
        L.c2 += ds5 * dl5 + ds6 * dl6;
        L.P1[2 * N] += -i5 + i6;
        L.P2[2 * N] += -(ds5 * dl5) * i5 + (ds6 * dl6) * i6;
    }
    L.amax = L.amax > 0.0 ? rcp1(L.amax) : 1e300;
    if (sl[SL.SC + 11] != 0.0) {
        // re-centring step of a warm solve: no second-order term.  The final-direction passes rebuild it from the AFFINE direction
        // of the lane's unknowns and of x (border_sigma clears that one): a zero affine direction makes it vanish there too.
#pragma unroll
        for (int k = 0; k < 2 * D::N2 + 1; ++k) L.P2[k] = 0;
#pragma unroll
        for (int k = 0; k < D::NW; ++k) L.dpa[k] = 0;
    }
    if (L.role == BORDER) {
        using BI = BorderIdx<N>;
        double ssoc[D::Q];
        ssoc[0] = sl[SlotLayout<N>::SC + 3];
        (sl + SlotLayout<N>::DSSA)[0] = (sl + SlotLayout<N>::DBA)[BI::TT];
#pragma unroll
        for (int k = 0; k < N; ++k) { ssoc[1 + k] = L.p[k] - L.p[N + k]; (sl + SlotLayout<N>::DSSA)[1 + k] = L.dpa[k] - L.dpa[N + k]; }
#pragma unroll
        for (int i = 0; i < D::Q; ++i) {
            double a = -(sl + SlotLayout<N>::LSOC)[i];
#pragma unroll
            for (int k = 0; k < D::Q; ++k) a -= (sl + SlotLayout<N>::W2)[i * D::Q + k] * (sl + SlotLayout<N>::DSSA)[k];
            (sl + SlotLayout<N>::DLSA)[i] = a;
        }
        L.amax = fmin(L.amax, fmin(soc_max_step<D::Q>(ssoc, (sl + SlotLayout<N>::DSSA)), soc_max_step<D::Q>((sl + SlotLayout<N>::LSOC), (sl + SlotLayout<N>::DLSA))));
#pragma unroll
        for (int k = 0; k < D::Q; ++k) { L.c1 += ssoc[k] * (sl + SlotLayout<N>::DLSA)[k] + (sl + SlotLayout<N>::LSOC)[k] * (sl + SlotLayout<N>::DSSA)[k]; L.c2 += (sl + SlotLayout<N>::DSSA)[k] * (sl + SlotLayout<N>::DLSA)[k]; }
    }
}

// BORDER: centring parameter from the affine step
template <int N>
GCS_HD void border_sigma(Lane<N> &L, const WaveShared &S, const SlotLayout<N> &SL)
{
    using D = Dim<N>;
    if (L.role != BORDER || (L.fl & F_DONE) || (L.fl & F_SKIP)) return;
    double *sl = slot_ptr<N>(S, SL, L.slot);
    const double *sin = sl + SL.SIN, *sout = sl + SL.SOUT;
    const int deg = (4 * L.m + 2) * (L.d + 1) + 1;
    const bool first_warm = sl[SL.SC + 11] != 0.0;
    const double amax = fmin(L.amax, fmin(sin[D::R2_BASE], sout[D::R2_BASE]));
    const double c1 = L.c1 + sin[D::R2_BASE + 1] + sout[D::R2_BASE + 1], c2 = L.c2 + sin[D::R2_BASE + 2] + sout[D::R2_BASE + 2];
    const double al = fmin(1.0, amax);
    const double gap = sl[SlotLayout<N>::SC + 5] * deg;
    const double mu_aff = (gap + al * c1 + al * al * c2) * rcp((double)deg);
    double sig = mu_aff * rcp(sl[SlotLayout<N>::SC + 5]);
    sig = sig < 0 ? 0 : (sig > 1 ? 1 : sig);      // (gcs_math::centring spelled out: the call changes the generated code here)
    sig = sig * sig * sig;
    const double sm = first_warm ? sl[SL.SC + 8] : sig * sl[SlotLayout<N>::SC + 5];      // (warm solve, first step: towards mu_ref e)
    sl[SL.SC + 1] = sm;
    if (first_warm) {      // (no second-order term: see pass_B)
#pragma unroll
        for (int k = 0; k < D::N2; ++k) sl[SL.DXA + k] = 0.0;
    }
    // cone part of kappa: sigma mu s^{-1} - W^{-1}( lt \ ((W^{-1} ds_a) o (W dl_a)) )
    double ssoc[D::Q], a1[D::Q], a2[D::Q], pr[D::Q], qv[D::Q];
    ssoc[0] = sl[SlotLayout<N>::SC + 3];
#pragma unroll
    for (int k = 0; k < N; ++k) ssoc[1 + k] = L.p[k] - L.p[N + k];
#pragma unroll
    for (int i = 0; i < D::Q; ++i) {
        double u1 = 0, u2 = 0;
#pragma unroll
        for (int k = 0; k < D::Q; ++k) { u1 += (sl + SlotLayout<N>::WI)[i * D::Q + k] * (sl + SlotLayout<N>::DSSA)[k]; u2 += (sl + SlotLayout<N>::W)[i * D::Q + k] * (sl + SlotLayout<N>::DLSA)[k]; }
        a1[i] = u1; a2[i] = u2;
    }
    {   // pr = a1 o a2
        double dsum = 0;
#pragma unroll
        for (int k = 0; k < D::Q; ++k) dsum += a1[k] * a2[k];
        pr[0] = dsum;
#pragma unroll
        for (int k = 1; k < D::Q; ++k) pr[k] = a1[0] * a2[k] + a2[0] * a1[k];
    }
    {   // lt o qv = pr
        const double det = soc_det<D::Q>((sl + SlotLayout<N>::LT));
        double ld1 = 0;
#pragma unroll
        for (int k = 1; k < D::Q; ++k) ld1 += (sl + SlotLayout<N>::LT)[k] * pr[k];
        qv[0] = ((sl + SlotLayout<N>::LT)[0] * pr[0] - ld1) * rcp(det);
        const double ilt0 = rcp((sl + SlotLayout<N>::LT)[0]);
#pragma unroll
        for (int k = 1; k < D::Q; ++k) qv[k] = (pr[k] - qv[0] * (sl + SlotLayout<N>::LT)[k]) * ilt0;
    }
    const double smd = sm * rcp(soc_det<D::Q>(ssoc));
#pragma unroll
    for (int i = 0; i < D::Q; ++i) {
        double a = 0;
#pragma unroll
        for (int k = 0; k < D::Q; ++k) a += (sl + SlotLayout<N>::WI)[i * D::Q + k] * qv[k];
        (sl + SlotLayout<N>::KSOC)[i] = smd * (i == 0 ? ssoc[0] : -ssoc[i]) - (first_warm ? 0.0 : a);
    }
}

// all lanes: G'kappa = sigma mu P1 - P2 ; block lanes stage t1 = B(-(g0+gk)), X't1, gk_x
template <int N>
GCS_HD void corrector_rhs(Lane<N> &L, const WaveShared &S, const SlotLayout<N> &SL, int lane, double (&vals)[Dim<N>::R3_N])
{
    using D = Dim<N>;
#pragma unroll
    for (int k = 0; k < D::R3_N; ++k) vals[k] = 0;
    if (L.role == IDLE || (L.fl & F_DONE) || (L.fl & F_SKIP)) return;
    double *sl = slot_ptr<N>(S, SL, L.slot);
    const double sm = sl[SL.SC + 1];
#pragma unroll
    for (int k = 0; k < 2 * D::N2 + 1; ++k) L.gk[k] = sm * L.P1[k] - L.P2[k];
    if (L.role == BLOCK) {
        double r[D::NW], t1[D::NW], xt[D::N2];
#pragma unroll
        for (int k = 0; k < D::NW; ++k) r[k] = -(L.g0[k] + L.gk[k]);
        block_apply<N>(L, r, t1);
        XT_apply<N>(L, t1, xt);
#pragma unroll
        for (int k = 0; k < D::NW; ++k) vals[D::R3_T + k] = t1[k];
#pragma unroll
        for (int k = 0; k < D::N2; ++k) { vals[D::R3_XT + k] = xt[k]; vals[D::R3_GX + k] = L.gk[D::NW + k]; }
    }
}

template <int N>
GCS_HD void border_corrector_solve(Lane<N> &L, const WaveShared &S, const SlotLayout<N> &SL)
{
    using D = Dim<N>; using BI = BorderIdx<N>;
    if (L.role != BORDER || (L.fl & F_DONE) || (L.fl & F_SKIP)) return;
    double *sl = slot_ptr<N>(S, SL, L.slot);
    const double *sin = sl + SL.SIN, *sout = sl + SL.SOUT;
    double gb[D::NB];
#pragma unroll
    for (int k = 0; k < D::N2; ++k) gb[k] = REG_DELTA * (sl + SlotLayout<N>::BX)[k] + L.gk[D::NW + k] + sin[D::R3_BASE + D::R3_GX + k] + sout[D::R3_BASE + D::R3_GX + k];
#pragma unroll
    for (int k = 0; k < D::NW; ++k) gb[D::N2 + k] = L.g0[k] + L.gk[k];
#pragma unroll
    for (int k = 0; k < N; ++k) { gb[BI::Z1 + k] -= (sl + SlotLayout<N>::KSOC)[1 + k]; gb[BI::Z2 + k] += (sl + SlotLayout<N>::KSOC)[1 + k]; }
    gb[BI::TT] = 1.0 - (sl + SlotLayout<N>::KSOC)[0];
    double rp[2][D::NW];
#pragma unroll
    for (int k = 0; k < D::NW; ++k) {
        const double zeta = (k < D::N2) ? L.p[k] : L.yy;
        rp[0][k] = zeta - sin[D::R1_W + k];
        rp[1][k] = zeta - sout[D::R1_W + k];
    }
    GCS_STAMP(0);
    border_solve<N>(L, sl, SL, gb, sin + D::R3_BASE + D::R3_T, sout + D::R3_BASE + D::R3_T,
                    sin + D::R3_BASE + D::R3_XT, sout + D::R3_BASE + D::R3_XT, rp, (sl + SlotLayout<N>::DB), SL.DX,
                    [&](double (&r1)[D::NB1]) { chol_solve_lds<D::NB1>(sl + SL.MF, r1); });
    GCS_STAMP(11);
}

// PASS D / E: final direction: step bound (APPLY = false) or dual update by alpha (APPLY = true).
// kappa of a row is rebuilt from the affine direction: kappa = (sigma mu - ds_a dl_a) / s.
template <int N, int I, bool APPLY, int SDL>
GCS_HD void pass_DE_half(Lane<N> &L, const double *A, const double *bc, const double *x, const double *dxa,
                         const double *dx, double *la, double *lb, double *dA, double *dB, int MM, int lane, double sm, double alpha)
{
    rows_half<N, I>(L, A, bc, x, [&](int j, const double(&a)[N], double b, double sa, double sb) {
        GCS_DUAL_REFS(ra, rb);
        const double l_a = ra, l_b = rb;
        // the step bound needs 1/s and 1/l: both from one reciprocal of the product s l (~ the barrier parameter)
        const double ipa = APPLY ? 0.0 : rcp1(sa * l_a), ipb = APPLY ? 0.0 : rcp1(sb * l_b);
        const double isa = APPLY ? rcp1(sa) : l_a * ipa, isb = APPLY ? rcp1(sb) : l_b * ipb;
        const double Da = l_a * isa, Db = l_b * isb;
        double dsa0, dsb0, dsa, dsb;
        row_dir<N, I>(j, a, b, L.dpa, dxa, dsa0, dsb0);
        row_dir<N, I>(j, a, b, L.dp, dx, dsa, dsb);
        const double ka = (sm - dsa0 * (-l_a - Da * dsa0)) * isa, kb = (sm - dsb0 * (-l_b - Db * dsb0)) * isb;
        const double dla = ka - l_a - Da * dsa, dlb = kb - l_b - Db * dsb;
        if (APPLY) {
            ra = l_a + alpha * dla;
            rb = l_b + alpha * dlb;
        } else {
            if (SDL) {   // kept for the update pass
                dA[(I * MM + j) * WAVE + lane] = dla;
                dB[(I * MM + j) * WAVE + lane] = dlb;
            }
            // largest -ds/s and -dl/l; the step bound is the reciprocal (taken once, in pass_DE)
            L.amax = fmax(L.amax, fmax(fmax(-dsa * isa, -dla * (sa * ipa)), fmax(-dsb * isb, -dlb * (sb * ipb))));
        }
    });
}

// PASS E, facet rows, SDL = 1: duals += alpha * (direction stored by pass D)
template <int N, int I>
GCS_HD void pass_E_half(Lane<N> &L, double *la, double *lb, const double *dA, const double *dB, int MM, int lane, double alpha)
{
#if GCS_MFIX
#pragma unroll
    for (int j = 0; j < GCS_MFIX; ++j) {
#else
#pragma unroll 2
    for (int j = 0; j < L.m; ++j) {
#endif
        GCS_DUAL_REFS(ra, rb);
        ra += alpha * dA[(I * MM + j) * WAVE + lane];
        rb += alpha * dB[(I * MM + j) * WAVE + lane];
    }
}

template <int N, bool APPLY, int SDL>
GCS_HD void pass_DE(Lane<N> &L, const WaveShared &S, const SlotLayout<N> &SL, int lane, int par)
{
    using D = Dim<N>; using BI = BorderIdx<N>;
    if (L.role == IDLE || (L.fl & F_DONE) || (L.fl & F_SKIP)) return;
    double *sl = slot_ptr<N>(S, SL, L.slot);
    const double sm = sl[SL.SC + 1];
    const double alpha = APPLY ? sl[SL.SC + 0] : 0.0;
    if (!APPLY) {
        if (L.role == BORDER) {
#pragma unroll
            for (int k = 0; k < D::NW; ++k) L.dp[k] = (sl + SlotLayout<N>::DB)[D::N2 + k];
        } else {
            lane_direction<N>(L, sl, SL, false, L.dp);
        }
        L.amax = 0.0;   // largest ratio until converted below
    }
    const double *x = sl + SL.X + par * D::N2;
    if (APPLY && SDL) {
        pass_E_half<N, 0>(L, S.lamA, S.lamB, S.dlA, S.dlB, S.MM, lane, alpha);
        pass_E_half<N, 1>(L, S.lamA, S.lamB, S.dlA, S.dlB, S.MM, lane, alpha);
    } else {
        pass_DE_half<N, 0, APPLY, SDL>(L, sl + SL.A, sl + SL.B, x, sl + SL.DXA, sl + SL.DX, S.lamA, S.lamB, S.dlA, S.dlB, S.MM, lane, sm, alpha);
        pass_DE_half<N, 1, APPLY, SDL>(L, sl + SL.A, sl + SL.B, x, sl + SL.DXA, sl + SL.DX, S.lamA, S.lamB, S.dlA, S.dlB, S.MM, lane, sm, alpha);
    }
    {
        const double s5 = L.yy, s6 = 1.0 - L.yy;
        const double ip5 = APPLY ? 0.0 : rcp1(s5 * L.l5), ip6 = APPLY ? 0.0 : rcp1(s6 * L.l6);
        const double i5 = APPLY ? rcp1(s5) : L.l5 * ip5, i6 = APPLY ? rcp1(s6) : L.l6 * ip6;
        const double D5 = L.l5 * i5, D6 = L.l6 * i6;
        const double d50 = L.dpa[2 * N], d60 = -L.dpa[2 * N], d5 = L.dp[2 * N], d6 = -L.dp[2 * N];
        const double k5 = (sm - d50 * (-L.l5 - D5 * d50)) * i5, k6 = (sm - d60 * (-L.l6 - D6 * d60)) * i6;
        const double dl5 = k5 - L.l5 - D5 * d5, dl6 = k6 - L.l6 - D6 * d6;
        if (APPLY) {
            L.l5 += alpha * dl5; L.l6 += alpha * dl6;
        } else {
            L.amax = fmax(L.amax, fmax(fmax(-d5 * i5, -dl5 * (s5 * ip5)), fmax(-d6 * i6, -dl6 * (s6 * ip6))));
            L.amax = L.amax > 0.0 ? rcp1(L.amax) : 1e300;
        }
    }
    if (L.role == BORDER && !APPLY) {
        double ssoc[D::Q];
        ssoc[0] = sl[SlotLayout<N>::SC + 3];
        (sl + SlotLayout<N>::DSS)[0] = (sl + SlotLayout<N>::DB)[BI::TT];
#pragma unroll
        for (int k = 0; k < N; ++k) { ssoc[1 + k] = L.p[k] - L.p[N + k]; (sl + SlotLayout<N>::DSS)[1 + k] = L.dp[k] - L.dp[N + k]; }
#pragma unroll
        for (int i = 0; i < D::Q; ++i) {
            double a = (sl + SlotLayout<N>::KSOC)[i] - (sl + SlotLayout<N>::LSOC)[i];
#pragma unroll
            for (int k = 0; k < D::Q; ++k) a -= (sl + SlotLayout<N>::W2)[i * D::Q + k] * (sl + SlotLayout<N>::DSS)[k];
            (sl + SlotLayout<N>::DLS)[i] = a;
        }
        L.amax = fmin(L.amax, fmin(soc_max_step<D::Q>(ssoc, (sl + SlotLayout<N>::DSS)), soc_max_step<D::Q>((sl + SlotLayout<N>::LSOC), (sl + SlotLayout<N>::DLS))));
    }
    if (APPLY) {
        // primal update of the lane's own unknowns
#pragma unroll
        for (int k = 0; k < D::N2; ++k) L.p[k] += alpha * L.dp[k];
        L.yy += alpha * L.dp[2 * N];
        if (L.role == BORDER) {
            double *xn = sl + SL.X + (par ^ 1) * D::N2;
#pragma unroll
            for (int k = 0; k < D::N2; ++k) { (sl + SlotLayout<N>::BX)[k] += alpha * (sl + SlotLayout<N>::DB)[k]; xn[k] = (sl + SlotLayout<N>::BX)[k]; }
            sl[SlotLayout<N>::SC + 3] += alpha * (sl + SlotLayout<N>::DB)[BI::TT];
#pragma unroll
            for (int k = 0; k < D::Q; ++k) (sl + SlotLayout<N>::LSOC)[k] += alpha * (sl + SlotLayout<N>::DLS)[k];
#pragma unroll
            for (int k = 0; k < 2 * D::NW; ++k) sl[SL.NU + k] += alpha * sl[SL.DNU + k];
            L.iters += 1;
        }
    }
}

// BORDER: step length with the cone guard
template <int N>
GCS_HD void border_alpha(Lane<N> &L, const WaveShared &S, const SlotLayout<N> &SL)
{
    using D = Dim<N>;
    if (L.role != BORDER || (L.fl & F_DONE) || (L.fl & F_SKIP)) return;
    double *sl = slot_ptr<N>(S, SL, L.slot);
    const double amax = fmin(L.amax, fmin(sl[SL.SIN + D::R4_BASE], sl[SL.SOUT + D::R4_BASE]));
    double al = gcs_math::step_length(amax);
    double ssoc[D::Q];
    ssoc[0] = sl[SlotLayout<N>::SC + 3];
#pragma unroll
    for (int k = 0; k < N; ++k) ssoc[1 + k] = L.p[k] - L.p[N + k];
    for (int tries = 0; tries < 40; ++tries) {
        double s2[D::Q], l2[D::Q];
#pragma unroll
        for (int k = 0; k < D::Q; ++k) { s2[k] = ssoc[k] + al * (sl + SlotLayout<N>::DSS)[k]; l2[k] = (sl + SlotLayout<N>::LSOC)[k] + al * (sl + SlotLayout<N>::DLS)[k]; }
        if (soc_interior<D::Q>(s2) && soc_interior<D::Q>(l2)) break;
        al *= 0.7;
    }
    L.fl = (L.fl & ~F_STALLED) | (gcs_math::step_stalled(al) ? F_STALLED : 0);
    sl[SL.SC + 0] = al;
}


// ---------------------------------------------------------------------------------------------
// global-memory interface of the vertex step and the wave-level driver
// ---------------------------------------------------------------------------------------------
struct ControlView {   // the fields of gcsadmm_control_block the kernels read
    double rho, mu_scale;
    int status;
};

// First lane of a vertex group (1 border lane + d block lanes: d_in incoming, then d - d_in outgoing) placed at
// or after lane `cur` of a wavefront.  With `align` the group is moved up until neither side segment straddles
// a 16-lane row, so that the segmented reductions can use DPP row shifts; -1: does not fit into this wavefront.
// The host packers (create_plan.h, tests/hostemu/emu.cpp) and phase_setup share this rule.
GCS_HD int group_base(int cur, int d, int d_in, int align)
{
    const int d_out = d - d_in;
    if (!align || d_in > 16 || d_out > 16) return cur + d + 1 <= WAVE ? cur : -1;
    for (int base = cur; base + d + 1 <= WAVE; ++base) {
        const int i0 = base + 1, i1 = base + d_in, o0 = base + d_in + 1, o1 = base + d;
        const bool in_ok = d_in == 0 || (i0 >> 4) == (i1 >> 4), out_ok = d_out == 0 || (o0 >> 4) == (o1 >> 4);
        if (in_ok && out_ok) return base;
    }
    return -1;
}

template <class T> struct VertexArgs : gcsadmm_k::StepArgs<T> {
    int n_waves;
    int align_rows;             // groups placed by group_base(.., align = 1)
    const int *wave_slot_ptr;   // [n_waves+1] into wave_vtx
    const int *wave_vtx;        // vertex ids, grouped per wave
    int MM;
    // slowest-first dispatch (loop_kernels.h reorder_kernel): workgroup b of the launch runs wavefront wave_order[b]; every wavefront
    // leaves the number of Newton iterations it ran in wave_iters (both may be null: identity order, nothing recorded)
    const int *wave_order = nullptr;
    int *wave_iters = nullptr;
};

// vertex id / incidence slot / edge id of a lane from its slot and position in the group
template <int N, class T>
GCS_HD void lane_ids(const Lane<N> &L, int wave, const VertexArgs<T> &a, int &v, int &inc, int &edge)
{
    v = a.wave_vtx[a.wave_slot_ptr[wave] + L.slot];
    inc = 0; edge = 0;
    if (L.role == BLOCK) {
        const int lo = a.inc_ptr[v];
        edge = a.inc_edge[lo + L.glane - 1];
        inc = gcsadmm_k::state_column(a, lo, L.glane - 1, edge, L.out);
    }
}

template <int N, class T>
GCS_HD void phase_setup(Lane<N> &L, int lane, int wave, const VertexArgs<T> &a, const WaveShared &S, const SlotLayout<N> &SL)
{
    using D = Dim<N>;
    L.role = IDLE; L.slot = 0; L.d = 0; L.d_in = 0; L.glane = 0; L.m = 0;
    L.out = 0; L.fl = 0; L.iters = 0; L.status = -1; L.bad = 0; L.segmask = 0; L.seg_head = 0; L.seg_steps = 0; L.seg_rowok = 1;
    const int s0 = a.wave_slot_ptr[wave], s1 = a.wave_slot_ptr[wave + 1];
    int free_lane = 0;
    for (int s = s0; s < s1; ++s) {
        const int v = a.wave_vtx[s];
        const int lo = a.inc_ptr[v], d = a.inc_ptr[v + 1] - lo;
        const int base = group_base(free_lane, d, a.deg_in[v], a.align_rows);
        if (lane >= base && lane <= base + d) {
            L.slot = s - s0; L.d = d; L.d_in = a.deg_in[v]; L.glane = lane - base;
            L.m = a.poly_ptr[v + 1] - a.poly_ptr[v];
            if (L.glane == 0) L.role = BORDER;
            else {
                L.role = BLOCK;
                L.out = (L.glane - 1) >= L.d_in;
                // side segment of this block lane: incoming lanes [1, d_in], outgoing lanes [d_in+1, d]
                const int last = L.out ? d : L.d_in, first = L.out ? L.d_in + 1 : 1, len = last - first + 1;
                L.seg_head = L.glane == first;
                L.seg_rowok = ((base + first) >> 4) == ((base + last) >> 4);
                for (int k = 0; k < 6; ++k)
                    if (L.glane + (1 << k) <= last) L.segmask |= 1 << k;
                while ((1 << L.seg_steps) < len) ++L.seg_steps;
            }
        }
        free_lane = base + d + 1;
    }
    {
    }
    if (L.role == BORDER) {
        double *sl = slot_ptr<N>(S, SL, L.slot);
        const int vtx = a.wave_vtx[s0 + L.slot];
        const int p0 = a.poly_ptr[vtx];
        for (int j = 0; j < L.m; ++j) {
#pragma unroll
            for (int k = 0; k < N; ++k) sl[SL.A + j * N + k] = a.poly_A[(size_t)(p0 + j) * N + k];
            sl[SL.B + j] = a.poly_bc[p0 + j];
        }
#pragma unroll
        for (int k = 0; k < N; ++k) sl[SL.CEN + k] = a.center[(size_t)vtx * N + k];
#pragma unroll
        for (int k = 0; k < 16; ++k) sl[SL.SC + k] = 0.0;
        sl[SL.SC + 8] = gcs_ws::WS_COLD_REF;
    }
}

// ---- warm start (warm_start.h): the record of a lane's vertex; a lane owns unit `glane` of it (0 = the border lane) ----
template <int N, class T>
GCS_HD double *warm_record(const Lane<N> &L, int wave, const VertexArgs<T> &a)
{
    if (a.warm == nullptr || L.role == IDLE) return nullptr;
    return a.warm + a.warm_ptr[a.wave_vtx[a.wave_slot_ptr[wave] + L.slot]];
}
// the facet-row duals of half I of a lane <-> the record (order: type x half x facet)
template <int N, int I, bool STORE>
GCS_HD void warm_rows_half(Lane<N> &L, double *la, double *lb, int MM, int lane, float *lam)      // (f32 in the record: warm_start.h)
{
#if GCS_MFIX
    const int m = GCS_MFIX;
#pragma unroll
    for (int j = 0; j < GCS_MFIX; ++j) {
#else
    const int m = L.m;
    for (int j = 0; j < L.m; ++j) {
#endif
        GCS_DUAL_REFS(ra, rb);
        // (the two duals of a facet row as one 8-byte pair: one memory instruction per row and direction -- as two strided floats the
        //  generic instantiation, whose register file is full, spilled 20 B.  A vertex's record is only ever read by the program that
        //  wrote it, so the order inside the 4m floats is this program's own.)
        struct alignas(8) F2 { float a, b; };
        F2 *pr = reinterpret_cast<F2 *>(lam) + (I * m + j);
        if (STORE) { F2 v; v.a = (float)ra; v.b = (float)rb; *pr = v; }
        else { const F2 v = *pr; ra = (double)v.a; rb = (double)v.b; }
    }
}
template <int N, class T>
GCS_HD void warm_store(Lane<N> &L, int lane, int wave, const VertexArgs<T> &a, const WaveShared &S, const SlotLayout<N> &SL)
{
    using D = Dim<N>; using WR = gcs_ws::WRec<N>;
    double *rec = warm_record<N, T>(L, wave, a);
    if (rec == nullptr) return;
    double *un = rec + WR::UNITS + L.glane * WR::unit_stride(L.m);
#pragma unroll
    for (int k = 0; k < D::N2; ++k) un[WR::P + k] = L.p[k];
    un[WR::P + D::N2] = L.yy;
    un[WR::LB] = L.l5; un[WR::LB + 1] = L.l6;
    warm_rows_half<N, 0, true>(L, S.lamA, S.lamB, S.MM, lane, reinterpret_cast<float *>(un + WR::LAM));
    warm_rows_half<N, 1, true>(L, S.lamA, S.lamB, S.MM, lane, reinterpret_cast<float *>(un + WR::LAM));
    if (L.role == BLOCK) {
#pragma unroll
        for (int k = 0; k < N; ++k) { un[WR::TG + k] = L.T1[k]; un[WR::TG + N + k] = L.T2[k]; }
        un[WR::TG + 2 * N] = L.Ty;
    } else {
        const double *sl = slot_ptr<N>(S, SL, L.slot);
#pragma unroll
        for (int k = 0; k < D::N2; ++k) rec[WR::XV + k] = (sl + SlotLayout<N>::BX)[k];
#pragma unroll
        for (int k = 0; k < 2 * D::NW; ++k) rec[WR::NU + k] = sl[SL.NU + k];
        rec[1] = sl[SL.SC + 13];      // rho of this solve
        rec[0] = 1.0;
    }
}

// targets of the block lanes; how far they moved since the vertex's record (per lane, reduced over the group by the caller)
template <int N, class T>
GCS_HD void phase_targets(Lane<N> &L, int lane, int wave, const VertexArgs<T> &a, const WaveShared &S, const SlotLayout<N> &SL,
                          double mu_scale)
{
    using D = Dim<N>; using WR = gcs_ws::WRec<N>;
    (void)lane;
    L.scale0 = 0.0;
    if (L.role != BLOCK) return;
    int vtx, inc, edge;
    lane_ids<N, T>(L, wave, a, vtx, inc, edge);
    double Tw[D::NW];
#pragma unroll
    for (int w = 0; w < D::NW; ++w)
        Tw[w] = gcsadmm_k::consensus_target(a, w, edge, inc, mu_scale);
#pragma unroll
    for (int k = 0; k < N; ++k) {
        L.T1[k] = L.out ? Tw[k] : Tw[N + k];
        L.T2[k] = L.out ? Tw[N + k] : 0.0;
    }
    L.Ty = Tw[2 * N];
    const double *rec = warm_record<N, T>(L, wave, a);
    if (rec != nullptr) {
        const double *tg = rec + WR::UNITS + L.glane * WR::unit_stride(L.m) + WR::TG;
        double dt = fabs(L.Ty - tg[2 * N]);
#pragma unroll
        for (int k = 0; k < N; ++k) {
            dt = fmax(dt, fabs(L.T1[k] - tg[k]));
            if (L.out) dt = fmax(dt, fabs(L.T2[k] - tg[N + k]));
        }
        L.scale0 = dt;
    }
}

// border lane: does this solve restart from the record?  (flags in the slot scalars, read by the group in phase_start)
template <int N, class T>
GCS_HD void phase_decide(Lane<N> &L, int wave, const VertexArgs<T> &a, const WaveShared &S, const SlotLayout<N> &SL, double rho)
{
    using D = Dim<N>;
    if (L.role != BORDER) return;
    double *sl = slot_ptr<N>(S, SL, L.slot);
    sl[SL.SC + 13] = rho;
    const double *rec = warm_record<N, T>(L, wave, a);
    if (rec == nullptr) return;
    const bool comparable = rec[0] == 1.0 && rec[1] == rho;
    const double dT = comparable ? rho * fmax(sl[SL.SIN + D::R0_BASE], sl[SL.SOUT + D::R0_BASE]) : -1.0;
    sl[SL.SC + 14] = dT; sl[SL.SC + 15] = 0.0;        // (dT < 0: no comparable record) for ws_learn at the end of the solve
    if (comparable && dT <= gcs_ws::ws_theta(rec)) {
        sl[SL.SC + 7] = 1.0;
        sl[SL.SC + 8] = fmax(gcs_ws::WS_MU_MIN, gcs_ws::WS_KAPPA * dT);
    }
}

// start point of a solve: the record's iterate (flag SC + 7), or the strictly feasible point of oracle_solve_vertex
template <int N, class T>
GCS_HD void phase_start(Lane<N> &L, int lane, int wave, const VertexArgs<T> &a, const WaveShared &S, const SlotLayout<N> &SL)
{
    using D = Dim<N>; using WR = gcs_ws::WRec<N>;
    if (L.role == IDLE) return;
    double *sl = slot_ptr<N>(S, SL, L.slot);
    L.fl &= ~(F_SKIP | F_STALLED);
    if (sl[SL.SC + 7] != 0.0) {
        double *rec = warm_record<N, T>(L, wave, a);
        double *un = rec + WR::UNITS + L.glane * WR::unit_stride(L.m);
#pragma unroll
        for (int k = 0; k < D::N2; ++k) L.p[k] = un[WR::P + k];
        L.yy = un[WR::P + D::N2];
        L.l5 = un[WR::LB]; L.l6 = un[WR::LB + 1];
        warm_rows_half<N, 0, false>(L, S.lamA, S.lamB, S.MM, lane, reinterpret_cast<float *>(un + WR::LAM));
        warm_rows_half<N, 1, false>(L, S.lamA, S.lamB, S.MM, lane, reinterpret_cast<float *>(un + WR::LAM));
        L.fl &= ~F_FRESH;
        if (L.role == BORDER) {
#pragma unroll
            for (int k = 0; k < D::N2; ++k) {
                const double xk = rec[WR::XV + k];
                (sl + SlotLayout<N>::BX)[k] = xk; sl[SL.X + k] = xk; sl[SL.X + D::N2 + k] = xk;
            }
#pragma unroll
            for (int k = 0; k < 2 * D::NW; ++k) sl[SL.NU + k] = rec[WR::NU + k];
            // cone pair re-centred at mu_ref: t^2 - mu_ref t - |u|^2 = 0, lambda = (1, -u / t)
            const double mr = sl[SL.SC + 8];
            double uu = 0;
#pragma unroll
            for (int k = 0; k < N; ++k) { const double uk = L.p[k] - L.p[N + k]; uu += uk * uk; }
            const double tn = 0.5 * (mr + sqrt_nr(mr * mr + 4.0 * uu)), itn = rcp(tn);
            sl[SlotLayout<N>::SC + 3] = tn;
            (sl + SlotLayout<N>::LSOC)[0] = 1.0;
#pragma unroll
            for (int k = 0; k < N; ++k) (sl + SlotLayout<N>::LSOC)[1 + k] = -(L.p[k] - L.p[N + k]) * itn;
        }
        return;
    }
    L.fl |= F_FRESH;
#pragma unroll
    for (int k = 0; k < D::N2; ++k) L.p[k] = 0.0;
    if (L.role == BLOCK) L.yy = 0.5 / (double)(L.out ? (L.d - L.d_in) : L.d_in);
    else {
#pragma unroll
        for (int k = 0; k < D::N2; ++k) { (sl + SlotLayout<N>::BX)[k] = 0.0; sl[SL.X + k] = 0.0; sl[SL.X + D::N2 + k] = 0.0; }
#pragma unroll
        for (int k = 0; k < 2 * D::NW; ++k) sl[SL.NU + k] = 0.0;
        L.yy = 0.5; sl[SlotLayout<N>::SC + 3] = 1.0;
        (sl + SlotLayout<N>::LSOC)[0] = 1.0;
#pragma unroll
        for (int k = 1; k < D::Q; ++k) (sl + SlotLayout<N>::LSOC)[k] = 0.0;
    }
}

// Segmented reduction: the block lanes of one side of a vertex are consecutive lanes of the wavefront; a
// value is reduced over such a segment with a shuffle-down tree (EX::seg_reduce: lane i adds lane i + 2^k
// while that lane is still inside the segment) and the head lane of the segment stores the result into the
// vertex's slot (in-sum or out-sum array).  No LDS staging, no extra barrier.
//
// The wave-level program.  EX provides each(f) = run f(L, lane) for every lane, then a barrier,
// all(pred) = wave-wide vote, wave_max(f) = wave-wide integer maximum, seg_reduce = the segmented
// reduction, count(counters, fails, iters) = accumulate statistics.
template <int N, class T, int SDL, class EX>
GCS_HD void run_vertex_program(EX &ex, int wave, const VertexArgs<T> &a, const WaveShared &S, double rho, double mu_scale)
{
    using D = Dim<N>;
    const SlotLayout<N> SL(S.MM);
    ex.each([&](Lane<N> &L, int lane) { phase_setup<N, T>(L, lane, wave, a, S, SL); });
    ex.each([&](Lane<N> &L, int lane) { phase_targets<N, T>(L, lane, wave, a, S, SL, mu_scale); });
    // number of shuffle steps the widest side segment of this wavefront needs (wave-uniform)
    const int nsteps = ex.wave_max([&](Lane<N> &L) { return L.seg_steps; });
    // every side segment inside one 16-lane row (always so with one vertex per wavefront): the tree can use
    // DPP row shifts (VALU latency) instead of ds_bpermute (an LDS round trip per step)
    const bool rows = ex.all([&](Lane<N> &L) { return L.seg_rowok != 0; });
    // per-lane reduction target: the in- and out-sums of the lane's vertex
    auto red = [&](Lane<N> &L, auto &v, int base, int special, int op, bool contributes) {
        double *sl = slot_ptr<N>(S, SL, L.slot);
        ex.seg_reduce(L, v, sl + SL.SIN + base, sl + SL.SOUT + base, special, op, contributes, nsteps, rows);
    };
    // how far the targets moved since the record: max over the block lanes of each group; then the start point
    ex.each([&](Lane<N> &L, int) {
        double v[1] = {L.role == BLOCK ? L.scale0 : 0.0};
        red(L, v, D::R0_BASE, 0, 2, L.role == BLOCK);
    });
    ex.each([&](Lane<N> &L, int) { phase_decide<N, T>(L, wave, a, S, SL, rho); });
    ex.each([&](Lane<N> &L, int lane) { phase_start<N, T>(L, lane, wave, a, S, SL); });
    int it_done = 0;
    for (int it = 0;; ++it) {
        const int par = it & 1;
        it_done = it;
        // a vertex whose warm solve failed starts again cold (its lanes sat out the rest of the last iteration)
        if (!ex.all([&](Lane<N> &L) { return !(L.fl & F_SKIP); }))
            ex.each([&](Lane<N> &L, int lane) {
                if (!(L.fl & F_SKIP)) return;
                phase_start<N, T>(L, lane, wave, a, S, SL);      // (SC + 7 was cleared when the solve failed: the cold point)
                if (L.role == BORDER) { L.iters = 0; L.fl &= ~F_SAVED; slot_ptr<N>(S, SL, L.slot)[SL.SC + 10] = 0.0; }
            });
        // ---- round 1: rows, block factorisation, and the sums over each side (three chunks, each
        //      produced right before it is reduced with wave shuffles; one barrier at the end) ----
        ex.each([&](Lane<N> &L, int lane) {
            const bool act = L.role == BLOCK && !(L.fl & F_DONE);
            pass_A<N>(L, S, SL, lane, par, rho, a.eps_edge);
            {
                double v[D::R1A_N];
                block_chunk_A<N>(L, v, act);
                red(L, v, 0, -1, 0, act);
            }
            {
                double v[D::R1B_N];
                block_chunk_B<N>(L, v, act);
                red(L, v, D::R1_BX, -1, 0, act);
            }
            {
                double v[D::R1C_N];
                block_chunk_C<N>(L, v, act);
                red(L, v, D::R1_XBX, -1, 0, act);
            }
        });
        // ---- border: convergence, factorisation, affine solve ----
        ex.each([&](Lane<N> &L, int) { border_factor_and_affine<N, T>(L, S, SL, a.ipm_tol, a.ipm_max_iter, wave, a); });
        if (ex.all([&](Lane<N> &L) { return L.role == IDLE || slot_ptr<N>(S, SL, L.slot)[SL.SC + 2] != 0.0; })) break;
        // ---- affine step statistics ----
        ex.each([&](Lane<N> &L, int lane) {
            pass_B<N, T>(L, S, SL, lane, par, wave, a);
            const bool act = L.role == BLOCK && !(L.fl & F_DONE) && !(L.fl & F_SKIP);
            double v[D::R2_N] = {act ? L.amax : 1e300, act ? L.c1 : 0.0, act ? L.c2 : 0.0};
            red(L, v, D::R2_BASE, 0, 1, act);
        });
        ex.each([&](Lane<N> &L, int) { border_sigma<N>(L, S, SL); });
        // ---- corrector right-hand side and solve ----
        ex.each([&](Lane<N> &L, int lane) {
            double v3[D::R3_N];
            corrector_rhs<N>(L, S, SL, lane, v3);
            red(L, v3, D::R3_BASE, -1, 0, L.role == BLOCK && !(L.fl & F_DONE) && !(L.fl & F_SKIP));
        });
        ex.each([&](Lane<N> &L, int) { border_corrector_solve<N>(L, S, SL); });
        // ---- final direction: step bound ----
        ex.each([&](Lane<N> &L, int lane) {
            pass_DE<N, false, SDL>(L, S, SL, lane, par);
            const bool act = L.role == BLOCK && !(L.fl & F_DONE) && !(L.fl & F_SKIP);
            double v[1] = {act ? L.amax : 1e300};
            red(L, v, D::R4_BASE, 0, 1, act);
        });
        ex.each([&](Lane<N> &L, int) { border_alpha<N>(L, S, SL); });
        // ---- update ----
        ex.each([&](Lane<N> &L, int lane) { pass_DE<N, true, SDL>(L, S, SL, lane, par); });
    }
    if (a.wave_iters != nullptr) ex.note(a.wave_iters + wave, it_done);
    // ---- un-centre and write out ----
    ex.each([&](Lane<N> &L, int) {
        if (L.role == IDLE) return;
        const double *sl = slot_ptr<N>(S, SL, L.slot);
        const double *cen = sl + SL.CEN;
        // inner failure (iteration limit, a slack that left its cone): the vertex keeps its previous copy columns and
        // outputs -- the reference's intent at admm_solver_v3.py:524-538 -- and is counted
        if (sl[SL.SC + 6] != 0.0) {
            if (L.role == BORDER) ex.count(a.counters, 1, L.iters + (int)sl[SL.SC + 12]);
            return;
        }
        int vtx, inc, edge;
        lane_ids<N, T>(L, wave, a, vtx, inc, edge);
        if (L.role == BLOCK) {
#pragma unroll
            for (int k = 0; k < N; ++k) {
                const double o1 = L.p[k] + L.yy * cen[k], o2 = L.p[N + k] + L.yy * cen[k];
                // incoming block: the first coupled word is only penalised, the copy keeps its target (read again here)
                const double tfree = L.out ? 0.0 : gcsadmm_k::consensus_target(a, k, edge, inc, mu_scale);
                a.copy[(size_t)k * a.NI + inc] = (T)(L.out ? o1 : tfree);
                a.copy[(size_t)(N + k) * a.NI + inc] = (T)(L.out ? o2 : o1);
            }
            a.copy[(size_t)(2 * N) * a.NI + inc] = (T)L.yy;
        } else {
#pragma unroll
            for (int k = 0; k < N; ++k) {
                a.xv[(size_t)vtx * D::N2 + k] = (sl + SlotLayout<N>::BX)[k] + cen[k];
                a.xv[(size_t)vtx * D::N2 + N + k] = (sl + SlotLayout<N>::BX)[N + k] + cen[k];
                a.zv[(size_t)vtx * D::N2 + k] = L.p[k] + L.yy * cen[k];
                a.zv[(size_t)vtx * D::N2 + N + k] = L.p[N + k] + L.yy * cen[k];
            }
            a.yv[vtx] = L.yy;
            ex.count(a.counters, 0, L.iters + (int)sl[SL.SC + 12]);
            double *rec = warm_record<N, T>(L, wave, a);
            if (rec != nullptr) gcs_ws::ws_learn(rec, sl[SL.SC + 7] != 0.0, sl[SL.SC + 15] != 0.0, sl[SL.SC + 14], L.iters);
        }
    });
}

#undef GCS_AMUL
#undef GCS_AMUL2
} // namespace GCS_NS
