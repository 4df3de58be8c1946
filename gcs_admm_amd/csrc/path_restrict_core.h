// path_restrict_core.h -- the convex restriction along a fixed path (rounding.solve_path_restriction), one path per 64-lane workgroup.
//
// For a path through regions r_0 .. r_{k-1}: points q_0 .. q_k in R^n, one epigraph variable t_j per segment,
//   min sum_j t_j   s.t.  A_r q_j <= b_r  for r = r_{j-1} (j >= 1) and r = r_j (j <= k-1),   (t_j, q_{j+1} - q_j) in Q^{n+1}.
// The method is that of gcs_admm_amd/conic.py (solve_socp), statement for statement: primal-dual interior point from a strictly
// feasible start (t_j = |q_{j+1} - q_j| + 1, row duals 1 / s, cone duals J s / det s), Nesterov-Todd scaling of the segment cones,
// Mehrotra predictor-corrector with both directions from one factorisation, sigma = (mu_aff / mu)^3, step min(1, 0.99 amax) shortened by
// 0.7 until every slack and dual is strictly inside, stop on mu <= tol.
//
// What conic.py solves as one dense system is a chain here.  With the unknowns ordered (q_0, t_0, q_1, t_1, .., q_k) every constraint
// couples one block or two consecutive blocks, so K = G' D G + reg I is symmetric block-tridiagonal with (n+1) x (n+1) blocks (the last
// block has no t: a unit diagonal in its place):
//   diagonal j     : [A' (lam / s) A + M11(j) + M11(j-1) + reg I,  -m0(j);  -m0(j)',  m00(j) + reg]
//   sub-diagonal j : rows of block j+1, columns of block j: [-M11(j), m0(j); 0, 0]
// where W_j^{-2} = [m00, m0'; m0, M11] = eta^-2 (2 u u' - J), u = J wb, of segment j's cone.  It is factored by a block Cholesky along
// the path, S_0 = H_00, Y_j = L_j^{-1} H_{j,j+1}, S_{j+1} = H_{j+1,j+1} - Y_j' Y_j with S_j = L_j L_j', and solved by a forward and a
// backward sweep, twice per Newton iteration.
//
// Arithmetic: gcs_math.h where it fits -- the refined reciprocals and roots, soc_det / soc_interior / soc_max_step / soc_scaling_wb,
// pivot_floor, centring, step_length.  Where it does not, because conic.py is the yardstick the costs are held to:
//   * the Tikhonov term is conic.py's reg = 1e-10 on the diagonal of K only (REG_DELTA = 1e-7 is part of the vertex objective and
//     would move the optimum by more than the bound the exact cases are held to);
//   * the stop is mu <= tol alone (mu_converged also accepts 1e3 tol after a stalled step), and a step below 1e-8 ends the solve as
//     failed unless mu <= tol (step_stalled's 1e-3 is the vertex solvers' rule).
//
// Written against an executor EX, as terminal_region.h is: tid, nthreads, sync, reduce3 (min, sum, sum: every lane gets the result,
// so the control flow below is uniform without a shared flag), and task(u, count): the task a lane runs at position u of a strided
// loop -- u itself on the device; the host build (tests/hostemu/restrict_emu.cpp) runs the tasks of a phase one after the other,
// forwards or backwards.  sync() orders GLOBAL memory: values written by one lane and read by another in a later phase cross the
// workspace, so the device executor waits for vmcnt(0) before its barrier.
//
// Workspace (restrict_ws_doubles, owned by the call): laid out by point, arr[component][point], so that consecutive lanes touch
// consecutive points, rows or segments.  The chain is the dependent path: it runs on lane 0, on blocks that all lanes stage through
// LDS CHUNK blocks at a time (coalesced loads and stores; lane 0 sees LDS latency only).
#pragma once
#include <stdint.h>

#include "gcs_math.h"

namespace gcs_restrict {

using gcs_math::rcp;

constexpr double RESTRICT_REG = 1e-10;   // conic.py reg
constexpr double STEP_MIN = 1e-8;        // conic.py: a step shorter than this ends the iteration
constexpr int BACKTRACKS = 40;
constexpr int CHUNK = 32;                // blocks of the chain staged in LDS at a time

// status of a path
constexpr int ST_CONVERGED = 0, ST_START_OUTSIDE = 1, ST_FAILED = -1;

// doubles of one path's workspace: k regions, R rows over its k + 1 points
GCS_HD long long restrict_ws_doubles(int n, long long k, long long R)
{
    const long long Q = n + 1, NP = k + 1;
    return n * NP + k + 6 * R + k * (7 * Q + 1) + Q * Q * NP + Q * Q * k + Q * NP;
}

template <int N> struct PathShared {
    static constexpr int B = N + 1;
    double Hs[CHUNK * B * B], Os[CHUNK * B * B], zs[CHUNK * B];      // diagonal blocks, coupling blocks, right-hand sides of a chunk
    double Yp[B * B], zp[B], ref[B];                                  // the coupling block / the solution next to the chunk; pivot references
};

struct PathProblem {
    int k;                      // regions on the path (>= 1); k + 1 points
    const int *poly;            // [k] region of every step
    const int *rowp;            // [k + 2] rows before point j; rowp[k + 1] = R
    const int *poly_ptr;        // the scene's CSR
    const double *A, *b;
    const double *start;        // [k + 1][n]
    double *points;             // [k + 1][n]
    double tol;
    int max_iter;
};

// point of row task u: the largest j with rowp[j] <= u
GCS_HD int row_point(const int *rowp, int NP, int u)
{
    int lo = 0, hi = NP;
    while (hi - lo > 1) { const int mid = (lo + hi) >> 1; if (rowp[mid] <= u) lo = mid; else hi = mid; }
    return lo;
}
// row of the scene behind local row l of point j: the rows of r_{j-1} come first, then those of r_j
GCS_HD int scene_row(const PathProblem &P, int j, int l)
{
    if (j >= 1) {
        const int r = P.poly[j - 1], m1 = P.poly_ptr[r + 1] - P.poly_ptr[r];
        if (l < m1) return P.poly_ptr[r] + l;
        l -= m1;
    }
    return P.poly_ptr[P.poly[j]] + l;
}

// y = Wbar x (inv: Wbar^{-1} x = J Wbar J x) for the unit hyperbolic vector wb; x and y may not alias
template <int Q> GCS_HD void apply_wbar(const double *wb, const double *x, double *y, bool inv)
{
    const double sg = inv ? -1.0 : 1.0;
    double d = 0;
#pragma unroll
    for (int c = 1; c < Q; ++c) d += wb[c] * x[c];
    y[0] = wb[0] * x[0] + sg * d;
    const double f = sg * x[0] + d * rcp(1.0 + wb[0]);
#pragma unroll
    for (int c = 1; c < Q; ++c) y[c] = x[c] + f * wb[c];
}
// y = W^{-2} x = ie2 (2 u (u . x) - J x), u = J wb
template <int Q> GCS_HD void apply_w2inv(const double *wb, double ie2, const double *x, double *y)
{
    double d = wb[0] * x[0];
#pragma unroll
    for (int c = 1; c < Q; ++c) d -= wb[c] * x[c];
    y[0] = ie2 * (2.0 * wb[0] * d - x[0]);
#pragma unroll
    for (int c = 1; c < Q; ++c) y[c] = ie2 * (x[c] - 2.0 * wb[c] * d);
}

// One path.  Returns its status; *cost_out, *iters_out are the same in every lane.
template <int N, class EX>
GCS_HD int path_restrict_solve(EX &ex, const PathProblem &P, double *ws, PathShared<N> &sh, double *cost_out, int *iters_out)
{
    constexpr int Q = N + 1, B = N + 1, BB = B * B;
    const int k = P.k, NP = k + 1, NS = k, R = P.rowp[NP];
    const int tid = ex.tid(), nt = ex.nthreads();
    const double *const A = P.A, *const bv = P.b;
    double *const q = ws, *const tt = q + (size_t)N * NP;
    double *const sl = tt + NS, *const lam = sl + R, *const dd = lam + R, *const ds = dd + R, *const dl = ds + R, *const kap = dl + R;
    double *const cs = kap + R, *const cl = cs + (size_t)Q * NS, *const wbv = cl + (size_t)Q * NS, *const cv = wbv + (size_t)Q * NS;
    double *const cc = cv + (size_t)Q * NS, *const cds = cc + (size_t)Q * NS, *const cdl = cds + (size_t)Q * NS, *const ie2v = cdl + (size_t)Q * NS;
    double *const Hd = ie2v + NS, *const Ho = Hd + (size_t)BB * NP, *const dw = Ho + (size_t)BB * NS;
    const int deg = R + NS;

    auto load_seg = [&](const double *arr, int j, double *x) {
#pragma unroll
        for (int c = 0; c < Q; ++c) x[c] = arr[(size_t)c * NS + j];
    };
    auto store_seg = [&](double *arr, int j, const double *x) {
#pragma unroll
        for (int c = 0; c < Q; ++c) arr[(size_t)c * NS + j] = x[c];
    };
    // entries of W_s^{-2} of segment s: (1 + a, 1 + c), and (1 + a, 0)
    auto Mqq = [&](int s, int a, int c) { return ie2v[s] * (2.0 * wbv[(size_t)(1 + a) * NS + s] * wbv[(size_t)(1 + c) * NS + s] + (a == c ? 1.0 : 0.0)); };
    auto Mq0 = [&](int s, int a) { return -2.0 * ie2v[s] * wbv[s] * wbv[(size_t)(1 + a) * NS + s]; };

    // ---- the chain (lane 0), on chunks that every lane stages through LDS ----
    // factor: Hd <- L_j (lower triangle, reciprocal pivots on the diagonal), Ho <- Y_j = L_j^{-1} H_{j,j+1}
    auto chain_factor = [&]() {
        for (int j0 = 0; j0 < NP; j0 += CHUNK) {
            const int cnt = NP - j0 < CHUNK ? NP - j0 : CHUNK;
            for (int u = tid; u < BB * cnt; u += nt) {
                const int i = ex.task(u, BB * cnt), e = i / cnt, jj = i - e * cnt;
                sh.Hs[jj * BB + e] = Hd[(size_t)e * NP + j0 + jj];
                if (j0 + jj < NS) sh.Os[jj * BB + e] = Ho[(size_t)e * NS + j0 + jj];
            }
            ex.sync();
            if (tid == 0) {
                for (int jj = 0; jj < cnt; ++jj) {
                    double *S = sh.Hs + jj * BB, *Y = sh.Os + jj * BB;
                    const double *Yprev = jj > 0 ? Y - BB : sh.Yp;
                    for (int a = 0; a < B; ++a) sh.ref[a] = S[a * B + a];
                    if (j0 + jj > 0)
                        for (int a = 0; a < B; ++a)
                            for (int c = 0; c <= a; ++c) { double v = S[a * B + c]; for (int r = 0; r < B; ++r) v -= Yprev[r * B + a] * Yprev[r * B + c]; S[a * B + c] = v; }
                    for (int c = 0; c < B; ++c) {
                        double dj = S[c * B + c];
                        for (int r = 0; r < c; ++r) dj -= S[c * B + r] * S[c * B + r];
                        const double inv = gcs_math::rsqrt_nr(gcs_math::pivot_floor(dj, sh.ref[c]));
                        S[c * B + c] = inv;
                        for (int a = c + 1; a < B; ++a) {
                            double v = S[a * B + c];
                            for (int r = 0; r < c; ++r) v -= S[a * B + r] * S[c * B + r];
                            S[a * B + c] = v * inv;
                        }
                    }
                    if (j0 + jj < NS)
                        for (int c = 0; c < B; ++c)
                            for (int a = 0; a < B; ++a) { double v = Y[a * B + c]; for (int r = 0; r < a; ++r) v -= S[a * B + r] * Y[r * B + c]; Y[a * B + c] = v * S[a * B + a]; }
                }
                if (j0 + cnt - 1 < NS) for (int e = 0; e < BB; ++e) sh.Yp[e] = sh.Os[(cnt - 1) * BB + e];
            }
            ex.sync();
            for (int u = tid; u < BB * cnt; u += nt) {
                const int i = ex.task(u, BB * cnt), e = i / cnt, jj = i - e * cnt;
                Hd[(size_t)e * NP + j0 + jj] = sh.Hs[jj * BB + e];
                if (j0 + jj < NS) Ho[(size_t)e * NS + j0 + jj] = sh.Os[jj * BB + e];
            }
            ex.sync();
        }
    };
    auto stage_in = [&](int j0, int cnt) {
        for (int u = tid; u < BB * cnt; u += nt) {
            const int i = ex.task(u, BB * cnt), e = i / cnt, jj = i - e * cnt;
            sh.Hs[jj * BB + e] = Hd[(size_t)e * NP + j0 + jj];
            if (j0 + jj < NS) sh.Os[jj * BB + e] = Ho[(size_t)e * NS + j0 + jj];
            if (e < B) sh.zs[jj * B + e] = dw[(size_t)e * NP + j0 + jj];
        }
        ex.sync();
    };
    auto stage_out = [&](int j0, int cnt) {
        ex.sync();
        for (int u = tid; u < B * cnt; u += nt) {
            const int i = ex.task(u, B * cnt), e = i / cnt, jj = i - e * cnt;
            dw[(size_t)e * NP + j0 + jj] = sh.zs[jj * B + e];
        }
        ex.sync();
    };
    // solve in place: dw <- K^{-1} dw
    auto chain_solve = [&]() {
        for (int j0 = 0; j0 < NP; j0 += CHUNK) {           // L z = r
            const int cnt = NP - j0 < CHUNK ? NP - j0 : CHUNK;
            stage_in(j0, cnt);
            if (tid == 0) {
                for (int jj = 0; jj < cnt; ++jj) {
                    const double *L = sh.Hs + jj * BB;
                    double *z = sh.zs + jj * B;
                    if (j0 + jj > 0) {
                        const double *Yprev = jj > 0 ? sh.Os + (jj - 1) * BB : sh.Yp, *zprev = jj > 0 ? z - B : sh.zp;
                        for (int c = 0; c < B; ++c) { double v = z[c]; for (int r = 0; r < B; ++r) v -= Yprev[r * B + c] * zprev[r]; z[c] = v; }
                    }
                    for (int a = 0; a < B; ++a) { double v = z[a]; for (int r = 0; r < a; ++r) v -= L[a * B + r] * z[r]; z[a] = v * L[a * B + a]; }
                }
                for (int c = 0; c < B; ++c) sh.zp[c] = sh.zs[(cnt - 1) * B + c];
                if (j0 + cnt - 1 < NS) for (int e = 0; e < BB; ++e) sh.Yp[e] = sh.Os[(cnt - 1) * BB + e];
            }
            stage_out(j0, cnt);
        }
        for (int j0 = ((NP - 1) / CHUNK) * CHUNK; j0 >= 0; j0 -= CHUNK) {      // L' x = z
            const int cnt = NP - j0 < CHUNK ? NP - j0 : CHUNK;
            stage_in(j0, cnt);
            if (tid == 0) {
                for (int jj = cnt - 1; jj >= 0; --jj) {
                    const double *L = sh.Hs + jj * BB, *Y = sh.Os + jj * BB;
                    double *x = sh.zs + jj * B;
                    if (j0 + jj < NS) {
                        const double *xnext = jj + 1 < cnt ? x + B : sh.zp;
                        for (int a = 0; a < B; ++a) { double v = x[a]; for (int c = 0; c < B; ++c) v -= Y[a * B + c] * xnext[c]; x[a] = v; }
                    }
                    for (int a = B - 1; a >= 0; --a) { double v = x[a]; for (int r = a + 1; r < B; ++r) v -= L[r * B + a] * x[r]; x[a] = v * L[a * B + a]; }
                }
                for (int c = 0; c < B; ++c) sh.zp[c] = sh.zs[c];
            }
            stage_out(j0, cnt);
        }
    };

    // One Newton direction for the targets sm (sigma mu) and, in the corrector, the second-order terms left by the predictor in kap
    // (rows) and cc (cones).  Leaves dw, ds, dl, cds, cdl; returns the step bound and the two sums of the step-length model
    // gap(al) = gap + al c1 + al^2 c2.  The predictor leaves its second-order terms behind.
    auto direction = [&](bool corrector, double sm, double &amax, double &c1, double &c2) {
        // v = lam + t of conic.py's direction(): rows (sm - corr) / s, cones lam + W^{-1} (lt \ (sm e - lt o lt - corr))
        for (int u = tid; u < R; u += nt) { const int i = ex.task(u, R); kap[i] = corrector ? (sm - kap[i]) * rcp(sl[i]) : 0.0; }
        for (int u = tid; u < NS; u += nt) {
            const int j = ex.task(u, NS);
            double wb[Q], l[Q], lt[Q], d[Q], x[Q], y[Q];
            load_seg(wbv, j, wb); load_seg(cl, j, l);
            const double ie = gcs_math::sqrt_nr(ie2v[j]), eta = rcp(ie);
            apply_wbar<Q>(wb, l, lt, false);
            double ll = 0;
#pragma unroll
            for (int c = 0; c < Q; ++c) { lt[c] *= eta; ll += lt[c] * lt[c]; }
            d[0] = sm - ll;
#pragma unroll
            for (int c = 1; c < Q; ++c) d[c] = -2.0 * lt[0] * lt[c];
            if (corrector) {
#pragma unroll
                for (int c = 0; c < Q; ++c) d[c] -= cc[(size_t)c * NS + j];
            }
            // lt o x = d
            double ld = 0;
#pragma unroll
            for (int c = 1; c < Q; ++c) ld += lt[c] * d[c];
            x[0] = (lt[0] * d[0] - ld) * rcp(gcs_math::soc_det<Q>(lt));
            const double il0 = rcp(lt[0]);
#pragma unroll
            for (int c = 1; c < Q; ++c) x[c] = (d[c] - x[0] * lt[c]) * il0;
            apply_wbar<Q>(wb, x, y, true);
#pragma unroll
            for (int c = 0; c < Q; ++c) y[c] = l[c] + ie * y[c];
            store_seg(cv, j, y);
        }
        ex.sync();
        // right-hand side -c - G' v, one (component, block) per task
        for (int u = tid; u < B * NP; u += nt) {
            const int i = ex.task(u, B * NP), c = i / NP, j = i - c * NP;
            double v;
            if (c < N) {
                v = 0;
                for (int r = P.rowp[j]; r < P.rowp[j + 1]; ++r) v -= A[(size_t)scene_row(P, j, r - P.rowp[j]) * N + c] * kap[r];
                if (j < NS) v -= cv[(size_t)(1 + c) * NS + j];
                if (j >= 1) v += cv[(size_t)(1 + c) * NS + j - 1];
            } else v = j < NS ? cv[j] - 1.0 : 0.0;
            dw[i] = v;
        }
        ex.sync();
        chain_solve();
        double am = 1e300, s1 = 0, s2 = 0;
        for (int u = tid; u < R; u += nt) {
            const int i = ex.task(u, R), j = row_point(P.rowp, NP, i), g = scene_row(P, j, i - P.rowp[j]);
            double adq = 0;
#pragma unroll
            for (int c = 0; c < N; ++c) adq += A[(size_t)g * N + c] * dw[(size_t)c * NP + j];
            const double sv = sl[i], lv = lam[i], dsv = -adq, dlv = kap[i] - lv - dd[i] * dsv;
            ds[i] = dsv; dl[i] = dlv;
            if (dsv < 0) am = fmin(am, -sv * rcp(dsv));
            if (dlv < 0) am = fmin(am, -lv * rcp(dlv));
            s1 += sv * dlv + lv * dsv; s2 += dsv * dlv;
            if (!corrector) kap[i] = dsv * dlv;
        }
        for (int u = tid; u < NS; u += nt) {
            const int j = ex.task(u, NS);
            double wb[Q], s[Q], l[Q], dsv[Q], dlv[Q], y[Q];
            load_seg(wbv, j, wb); load_seg(cs, j, s); load_seg(cl, j, l);
            dsv[0] = dw[(size_t)N * NP + j];
#pragma unroll
            for (int c = 0; c < N; ++c) dsv[1 + c] = dw[(size_t)c * NP + j + 1] - dw[(size_t)c * NP + j];
            apply_w2inv<Q>(wb, ie2v[j], dsv, y);
#pragma unroll
            for (int c = 0; c < Q; ++c) dlv[c] = cv[(size_t)c * NS + j] - l[c] - y[c];
            store_seg(cds, j, dsv); store_seg(cdl, j, dlv);
            am = fmin(am, fmin(gcs_math::soc_max_step<Q>(s, dsv), gcs_math::soc_max_step<Q>(l, dlv)));
#pragma unroll
            for (int c = 0; c < Q; ++c) { s1 += s[c] * dlv[c] + l[c] * dsv[c]; s2 += dsv[c] * dlv[c]; }
            if (!corrector) {       // (W^{-1} ds) o (W dl)
                const double ie = gcs_math::sqrt_nr(ie2v[j]), eta = rcp(ie);
                double a1[Q], a2[Q];
                apply_wbar<Q>(wb, dsv, a1, true); apply_wbar<Q>(wb, dlv, a2, false);
                double dot = 0;
#pragma unroll
                for (int c = 0; c < Q; ++c) { a1[c] *= ie; a2[c] *= eta; dot += a1[c] * a2[c]; }
                y[0] = dot;
#pragma unroll
                for (int c = 1; c < Q; ++c) y[c] = a1[0] * a2[c] + a2[0] * a1[c];
                store_seg(cc, j, y);
            }
        }
        ex.reduce3(am, s1, s2);
        amax = am; c1 = s1; c2 = s2;
    };

    // ---- the start ----
    for (int u = tid; u < N * NP; u += nt) { const int i = ex.task(u, N * NP), c = i / NP, j = i - c * NP; q[i] = P.start[(size_t)j * N + c]; }
    ex.sync();
    for (int u = tid; u < NS; u += nt) {
        const int j = ex.task(u, NS);
        double nn = 0;
#pragma unroll
        for (int c = 0; c < N; ++c) { const double d = q[(size_t)c * NP + j + 1] - q[(size_t)c * NP + j]; nn += d * d; }
        tt[j] = gcs_math::sqrt_nr(nn) + 1.0;
    }
    ex.sync();

    int status = ST_FAILED, it = 0;
    bool vanished = false;
    for (it = 0;; ++it) {
        // ---- slacks, complementarity, scaling of the cones
        double flag = 1.0, gap = 0, unused = 0;
        for (int u = tid; u < R; u += nt) {
            const int i = ex.task(u, R), j = row_point(P.rowp, NP, i), g = scene_row(P, j, i - P.rowp[j]);
            double a = bv[g];
#pragma unroll
            for (int c = 0; c < N; ++c) a -= A[(size_t)g * N + c] * q[(size_t)c * NP + j];
            sl[i] = a;
            if (!(a > 0)) flag = -1.0;
            const double ia = rcp(a);
            if (it == 0) lam[i] = ia;
            const double lv = lam[i];
            if (!(lv > 0)) flag = -1.0;
            gap += a * lv;
            dd[i] = lv * ia;
        }
        for (int u = tid; u < NS; u += nt) {
            const int j = ex.task(u, NS);
            double s[Q], l[Q], wb[Q], eta = 1.0;
            s[0] = tt[j];
#pragma unroll
            for (int c = 0; c < N; ++c) s[1 + c] = q[(size_t)c * NP + j + 1] - q[(size_t)c * NP + j];
            store_seg(cs, j, s);
            if (!gcs_math::soc_interior<Q>(s)) { flag = -1.0; continue; }
            if (it == 0) {
                const double idet = rcp(gcs_math::soc_det<Q>(s));
                l[0] = s[0] * idet;
#pragma unroll
                for (int c = 1; c < Q; ++c) l[c] = -s[c] * idet;
                store_seg(cl, j, l);
            } else load_seg(cl, j, l);
#pragma unroll
            for (int c = 0; c < Q; ++c) gap += s[c] * l[c];
            if (!(l[0] > 0) || !gcs_math::soc_scaling_wb<Q>(s, l, wb, eta)) { flag = -1.0; continue; }
            store_seg(wbv, j, wb);
            ie2v[j] = rcp(eta * eta);
        }
        ex.reduce3(flag, gap, unused);
        if (flag < 0) { status = it == 0 ? ST_START_OUTSIDE : ST_FAILED; break; }
        const double mu = gap / deg;
        if (mu <= P.tol) { status = ST_CONVERGED; break; }
        if (!(mu > P.tol) || it >= P.max_iter || vanished) break;      // non-finite, iteration limit, vanished step
        ex.sync();
        // ---- block assembly, one (entry, block) per task; the coupling blocks are stored transposed (rows of block j)
        for (int u = tid; u < BB * NP; u += nt) {
            const int i = ex.task(u, BB * NP), e = i / NP, j = i - e * NP, a = e / B, c = e - a * B;
            double v;
            if (a < N && c < N) {
                v = a == c ? RESTRICT_REG : 0.0;
                for (int r = P.rowp[j]; r < P.rowp[j + 1]; ++r) {
                    const size_t g = (size_t)scene_row(P, j, r - P.rowp[j]) * N;
                    v += dd[r] * A[g + a] * A[g + c];
                }
                if (j < NS) v += Mqq(j, a, c);
                if (j >= 1) v += Mqq(j - 1, a, c);
            } else if (a == N && c == N) {
                v = j < NS ? ie2v[j] * (2.0 * wbv[j] * wbv[j] - 1.0) + RESTRICT_REG : 1.0;
            } else {
                v = j < NS ? -Mq0(j, a < N ? a : c) : 0.0;
            }
            Hd[i] = v;
        }
        for (int u = tid; u < BB * NS; u += nt) {
            const int i = ex.task(u, BB * NS), e = i / NS, j = i - e * NS, a = e / B, c = e - a * B;
            double v = 0.0;         // (a: unknown of block j, c: unknown of block j + 1)
            if (c < N) v = a < N ? -Mqq(j, a, c) : Mq0(j, c);
            Ho[i] = v;
        }
        ex.sync();
        chain_factor();
        // ---- predictor, centring, corrector
        double amax, c1, c2;
        direction(false, 0.0, amax, c1, c2);
        const double al_aff = fmin(1.0, amax);
        const double sm = gcs_math::centring((gap + al_aff * c1 + al_aff * al_aff * c2) / (deg * mu)) * mu;
        ex.sync();
        direction(true, sm, amax, c1, c2);
        double al = gcs_math::step_length(amax);
        for (int tries = 0; tries < BACKTRACKS; ++tries) {      // every slack and dual strictly inside despite round-off
            double ok = 1.0, u1 = 0, u2 = 0;
            for (int u = tid; u < R; u += nt) {
                const int i = ex.task(u, R);
                if (!(sl[i] + al * ds[i] > 0) || !(lam[i] + al * dl[i] > 0)) ok = -1.0;
            }
            for (int u = tid; u < NS; u += nt) {
                const int j = ex.task(u, NS);
                double s2[Q], l2[Q];
#pragma unroll
                for (int c = 0; c < Q; ++c) {
                    s2[c] = cs[(size_t)c * NS + j] + al * cds[(size_t)c * NS + j];
                    l2[c] = cl[(size_t)c * NS + j] + al * cdl[(size_t)c * NS + j];
                }
                if (!gcs_math::soc_interior<Q>(s2) || !gcs_math::soc_interior<Q>(l2)) ok = -1.0;
            }
            ex.reduce3(ok, u1, u2);
            if (ok > 0) break;
            al *= 0.7;
        }
        for (int u = tid; u < N * NP; u += nt) { const int i = ex.task(u, N * NP); q[i] += al * dw[i]; }
        for (int u = tid; u < NS; u += nt) {
            const int j = ex.task(u, NS);
            tt[j] += al * dw[(size_t)N * NP + j];
#pragma unroll
            for (int c = 0; c < Q; ++c) cl[(size_t)c * NS + j] += al * cdl[(size_t)c * NS + j];
        }
        for (int u = tid; u < R; u += nt) { const int i = ex.task(u, R); lam[i] += al * dl[i]; }
        vanished = al < STEP_MIN;
        ex.sync();
    }
    // ---- the points, and the polyline length recomputed from them
    ex.sync();
    double big = 0, len = 0, unused = 0;
    for (int u = tid; u < N * NP; u += nt) { const int i = ex.task(u, N * NP), c = i / NP, j = i - c * NP; P.points[(size_t)j * N + c] = q[i]; }
    for (int u = tid; u < NS; u += nt) {
        const int j = ex.task(u, NS);
        double nn = 0;
#pragma unroll
        for (int c = 0; c < N; ++c) { const double d = q[(size_t)c * NP + j + 1] - q[(size_t)c * NP + j]; nn += d * d; }
        len += gcs_math::sqrt_nr(nn);
    }
    ex.reduce3(big, len, unused);
    *cost_out = status == ST_CONVERGED ? len : INFINITY;
    *iters_out = it;
    return status;
}

}  // namespace gcs_restrict
