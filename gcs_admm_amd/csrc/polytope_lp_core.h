// polytope_lp_core.h -- the per-lane LP solver of polytope_lp.hip (host + device: the host build exists for
// the lock-step debugging harness under tests/hostemu only; the product path is the HIP kernels).
#pragma once
#include <math.h>
#include <stddef.h>
#if defined(__HIPCC__)
#define GCS_LP_HD __host__ __device__ __forceinline__
#else
#define GCS_LP_HD inline
#endif

namespace gcsadmm_lp {

constexpr int WAVE = 64;
constexpr int MAX_IT = 80;
constexpr double R_CAP = 1e6;      // the inscribed radius is capped (unbounded sets)
constexpr double X_CAP = 1e8;      // coordinates are capped in the bounding LPs (unbounded directions)

// LDS of one workgroup: the duals and their directions of 64 LPs, [row][lane] each.  Rows per LP for a scene whose largest polytope
// has maxm rows: the polytope's and the cap on r (centres), both polytopes' and the cap (overlaps), the polytope's and 2n caps (bounds).
// An LP whose rows do not fit is refused by the launchers (GCSADMM_ERR_UNSUPPORTED), never truncated.
constexpr size_t LDS_MAX_BYTES = 160 * 1024;
GCS_LP_HD constexpr size_t lds_bytes(int rows) { return (size_t)2 * rows * WAVE * sizeof(double); }
GCS_LP_HD constexpr int centre_rows(int maxm) { return maxm + 1; }
GCS_LP_HD constexpr int overlap_rows(int maxm) { return 2 * maxm + 1; }
GCS_LP_HD constexpr int bounds_rows(int maxm, int n) { return maxm + 2 * n; }

GCS_LP_HD constexpr int PK(int i, int j) { return i >= j ? i * (i + 1) / 2 + j : j * (j + 1) / 2 + i; }

struct Polys {
    int n, P;
    const int *ptr;        // [P+1]
    const double *A;       // [rows][n]
    const double *b;       // [rows]
    const double *nrm;     // [rows]  |a_i|_2
};

// one LP:  min c'w  s.t.  g_i'w <= h_i ;  rows = rows of polytope p (+ polytope q) (+ caps)
template <int N, bool BALL> struct Rows {
    static constexpr int K = BALL ? N + 1 : N;
    const Polys &S;
    int p0, m1, q0, m2, m;
    GCS_LP_HD Rows(const Polys &s, int p, int q) : S(s)
    {
        p0 = s.ptr[p]; m1 = s.ptr[p + 1] - p0;
        q0 = q >= 0 ? s.ptr[q] : 0; m2 = q >= 0 ? s.ptr[q + 1] - q0 : 0;
        m = m1 + m2 + (BALL ? 1 : 2 * N);
    }
    GCS_LP_HD double norm(int i) const { return S.nrm[i < m1 ? p0 + i : q0 + (i - m1)]; }   // |a_i| of a polytope row, i < m1 + m2
    GCS_LP_HD void get(int i, double (&g)[K], double &h) const
    {
        if (i < m1 + m2) {
            const int r = i < m1 ? p0 + i : q0 + (i - m1);
#pragma unroll
            for (int k = 0; k < N; ++k) g[k] = S.A[(size_t)r * N + k];
            if (BALL) g[K - 1] = S.nrm[r];
            h = S.b[r];
        } else if (BALL) {
#pragma unroll
            for (int k = 0; k < N; ++k) g[k] = 0.0;
            g[K - 1] = 1.0; h = R_CAP;
        } else {
            const int j = i - (m1 + m2), k = j >> 1;
#pragma unroll
            for (int kk = 0; kk < N; ++kk) g[kk] = 0.0;
            g[k] = (j & 1) ? -1.0 : 1.0; h = X_CAP;
        }
    }
};

template <int K> GCS_LP_HD bool chol(double (&H)[K * (K + 1) / 2])
{
    bool ok = true;
#pragma unroll
    for (int j = 0; j < K; ++j) {
        double d = H[PK(j, j)];
#pragma unroll
        for (int k = 0; k < j; ++k) d -= H[PK(j, k)] * H[PK(j, k)];
        if (!(d > 0.0)) { ok = false; d = 1.0; }
        const double inv = 1.0 / sqrt(d);
        H[PK(j, j)] = inv;
#pragma unroll
        for (int i = j + 1; i < K; ++i) {
            double s = H[PK(i, j)];
#pragma unroll
            for (int k = 0; k < j; ++k) s -= H[PK(i, k)] * H[PK(j, k)];
            H[PK(i, j)] = s * inv;
        }
    }
    return ok;
}
template <int K> GCS_LP_HD void chol_solve(const double (&L)[K * (K + 1) / 2], double (&x)[K])
{
#pragma unroll
    for (int i = 0; i < K; ++i) {
        double s = x[i];
#pragma unroll
        for (int k = 0; k < i; ++k) s -= L[PK(i, k)] * x[k];
        x[i] = s * L[PK(i, i)];
    }
#pragma unroll
    for (int i = K - 1; i >= 0; --i) {
        double s = x[i];
#pragma unroll
        for (int k = i + 1; k < K; ++k) s -= L[PK(k, i)] * x[k];
        x[i] = s * L[PK(i, i)];
    }
}

// status: 0 converged, 1 stopped early with r > 0, 2 stopped early with the dual bound below -tol, -1 iteration limit, a start
// that is not strictly feasible, or a non-finite iterate (a non-finite result is never reported with a status >= 0).
// The duals start at lam = mu0 / s, where mu0 carries the units of the slacks (a length times |a|): the dual constraint fixes the
// duals at O(1 / |a|) whatever the size of the region, so they start at their own scale and the iteration is the same for a scene
// given in metres or in millimetres.
//   ball LP:   mu0 = 1 / sum_i |g_i,r| / s_i, with which the r component of the dual residual starts at zero;
//   bounds LP: mu0 = max(rho, 1), rho the distance of the start to its nearest polytope row -- not below lam = 1 / s: complementarity
//              and dual residual fall at the same rate (1 - step), the stop asks for 1e-11 and 1e-9 in absolute terms, and a region
//              of size 1e-6 started at mu = 1e-6 would have its slacks at 1e-15, below the round-off of b - a x a few hundred units
//              from the origin, before the dual residual has come down.
template <int N, bool BALL>
GCS_LP_HD int lp_ipm(const Rows<N, BALL> &R, const double (&c)[Rows<N, BALL>::K], double (&w)[Rows<N, BALL>::K],
                      double *lam, double *dlam, int lane, bool early, double tol, int *iters_out)
{
    constexpr int K = Rows<N, BALL>::K, KS = K * (K + 1) / 2;
    const int m = R.m;
    double g[K], h;
    bool interior = true;
    double v = 0.0, rho = 1e300;
    for (int i = 0; i < m; ++i) {
        R.get(i, g, h);
        double s = h;
#pragma unroll
        for (int k = 0; k < K; ++k) s -= g[k] * w[k];
        interior = interior && s > 0.0 && s < 1e300;
        if (BALL) v += g[K - 1] / s;
        else if (i < R.m1 + R.m2) rho = fmin(rho, s / R.norm(i));
        lam[i * WAVE + lane] = 1.0 / s;
    }
    const double mu0 = BALL ? 1.0 / v : fmax(rho, 1.0);
    interior = interior && mu0 > 0.0 && mu0 < 1e300;
    for (int i = 0; i < m; ++i) lam[i * WAVE + lane] *= mu0;    // duals on the central path of the start: lam = mu0 / s
    int status = -1, it = 0;
    double w_prev[K], mu_prev = 1e300, rd_prev = 1e300, al_prev = 0.0;
    bool retried = false;
#pragma unroll
    for (int k = 0; k < K; ++k) w_prev[k] = w[k];
    for (; interior && it < MAX_IT; ++it) {
        double H[KS], rd[K], gap = 0, hl = 0;
        bool lost = false;
#pragma unroll
        for (int k = 0; k < KS; ++k) H[k] = 0;
#pragma unroll
        for (int k = 0; k < K; ++k) rd[k] = c[k];
        for (int i = 0; i < m; ++i) {
            R.get(i, g, h);
            double s = h;
#pragma unroll
            for (int k = 0; k < K; ++k) s -= g[k] * w[k];
            const double l = lam[i * WAVE + lane], d = l / s;
            lost = lost || !(s > 0.0);
            gap += s * l; hl += h * l;
#pragma unroll
            for (int a = 0; a < K; ++a) {
                rd[a] += l * g[a];
#pragma unroll
                for (int b2 = 0; b2 <= a; ++b2) H[PK(a, b2)] += d * g[a] * g[b2];
            }
        }
        const double mu = gap / m;
        double rdmax = 0;
#pragma unroll
        for (int k = 0; k < K; ++k) rdmax = fmax(rdmax, fabs(rd[k]));
        if (lost) {   // the last step left a slack of 0.01 of its value, and b - a x of the new point lost it to round-off (slacks
                      // of 1e-12 on a region 3e4 from the origin).  Once: nine tenths of that step instead, which leaves a tenth of
                      // the slack.  Lost again: the point before the step is as good as f64 gets.
            if (retried || it == 0) {
#pragma unroll
                for (int k = 0; k < K; ++k) w[k] = w_prev[k];
                if (mu_prev <= 1e-7 * fmax(1.0, fabs(BALL ? w[K - 1] : 1.0)) && rd_prev <= 1e-7) status = 0;
                break;
            }
            retried = true;
#pragma unroll
            for (int k = 0; k < K; ++k) w[k] = w_prev[k] + 0.9 * (w[k] - w_prev[k]);
            for (int i = 0; i < m; ++i) lam[i * WAVE + lane] -= 0.1 * al_prev * dlam[i * WAVE + lane];
            continue;
        }
        retried = false;
        mu_prev = mu; rd_prev = rdmax;
#pragma unroll
        for (int k = 0; k < K; ++k) w_prev[k] = w[k];
        if (BALL && early) {
            if (w[K - 1] > 0.0) { status = 1; break; }                       // a point with a ball around it: they overlap
            // dual bound r* <= h'lam, valid up to the dual residual times |w*|: only used with a clear margin,
            // near-touching pairs run to convergence and are decided on r* itself
            if (rdmax <= 1e-9 && hl < -tol - 1e-6) { status = 2; break; }
        }
        const double mu_stop = 1e-11 * fmax(1.0, fabs(BALL ? w[K - 1] : 1.0));
        if (mu <= mu_stop && rdmax <= 1e-9) { status = 0; break; }
        double tr = 0;
#pragma unroll
        for (int k = 0; k < K; ++k) tr += H[PK(k, k)];
#pragma unroll
        for (int k = 0; k < K; ++k) H[PK(k, k)] += 1e-15 * tr;
        chol<K>(H);
        double dwa[K];
#pragma unroll
        for (int k = 0; k < K; ++k) dwa[k] = -c[k];
        chol_solve<K>(H, dwa);
        // affine step: bound and the complementarity it would leave
        double amax = 1e300, c1 = 0, c2 = 0;
        for (int i = 0; i < m; ++i) {
            R.get(i, g, h);
            double s = h, q = 0;
#pragma unroll
            for (int k = 0; k < K; ++k) { s -= g[k] * w[k]; q += g[k] * dwa[k]; }
            const double l = lam[i * WAVE + lane], d = l / s;
            const double dsa = -q, dla = -l + d * q;
            if (dsa < 0) amax = fmin(amax, -s / dsa);
            if (dla < 0) amax = fmin(amax, -l / dla);
            c1 += s * dla + l * dsa; c2 += dsa * dla;
        }
        const double ala = fmin(1.0, amax);
        double sig = (gap + ala * c1 + ala * ala * c2) / gap;
        sig = sig < 0 ? 0 : (sig > 1 ? 1 : sig);
        sig = sig * sig * sig;
        const double sm = sig * mu;
        double dw[K];
#pragma unroll
        for (int k = 0; k < K; ++k) dw[k] = -c[k];
        for (int i = 0; i < m; ++i) {
            R.get(i, g, h);
            double s = h, q = 0;
#pragma unroll
            for (int k = 0; k < K; ++k) { s -= g[k] * w[k]; q += g[k] * dwa[k]; }
            const double l = lam[i * WAVE + lane], d = l / s;
            const double dsa = -q, dla = -l + d * q;
            const double f = (sm - dsa * dla) / s;
#pragma unroll
            for (int k = 0; k < K; ++k) dw[k] -= g[k] * f;
        }
        chol_solve<K>(H, dw);
        amax = 1e300;
        for (int i = 0; i < m; ++i) {
            R.get(i, g, h);
            double s = h, q = 0, qa = 0;
#pragma unroll
            for (int k = 0; k < K; ++k) { s -= g[k] * w[k]; q += g[k] * dw[k]; qa += g[k] * dwa[k]; }
            const double l = lam[i * WAVE + lane], d = l / s;
            const double dsa = -qa, dla = -l + d * qa;
            const double ds = -q, dl = (sm - dsa * dla) / s - l + d * q;
            if (ds < 0) amax = fmin(amax, -s / ds);
            if (dl < 0) amax = fmin(amax, -l / dl);
            dlam[i * WAVE + lane] = dl;
        }
        const double al = fmin(1.0, 0.99 * amax);
        if (!(al > 1e-10)) {             // no progress (or a slack lost to round-off): the point is as good as f64 gets
            if (mu <= 1e-7 * fmax(1.0, fabs(BALL ? w[K - 1] : 1.0)) && rdmax <= 1e-7) status = 0;
            break;
        }
        for (int i = 0; i < m; ++i) lam[i * WAVE + lane] += al * dlam[i * WAVE + lane];
        al_prev = al;
#pragma unroll
        for (int k = 0; k < K; ++k) w[k] += al * dw[k];
    }
    if (iters_out) *iters_out = it;
#pragma unroll
    for (int k = 0; k < K; ++k)
        if (!(fabs(w[k]) < 1e300)) status = -1;
    return status;
}

// strictly feasible start of the ball LP from a point x0.  With t_i = (b_i - a_i x0) / |a_i| the signed distances of x0 to the rows,
// r0 lies below the tightest one by the size of the problem as x0 sees it -- max(|min t|, max t - min t) -- so that every slack
// t_i - r0 is of that one order, whatever the units of the scene, and however far outside x0 lies (the start of an overlap LP is the
// centre of ONE of the two regions).  A non-finite x0 is treated as no x0.
template <int N> GCS_LP_HD void ball_start(const Rows<N, true> &R, const double *x0, double (&w)[N + 1])
{
    double g[N + 1], h;
    bool given = x0 != nullptr;
#pragma unroll
    for (int k = 0; k < N; ++k) {
        w[k] = x0 ? x0[k] : 0.0;
        given = given && fabs(w[k]) < 1e300;
    }
    if (!given) {   // no start point given: the least-squares point of A x = b (near the middle of a bounded region,
                    // wherever it sits; starting at the origin costs iterations and digits when the region is far away)
        double G[N * (N + 1) / 2], t[N];
#pragma unroll
        for (int k = 0; k < N * (N + 1) / 2; ++k) G[k] = 0;
#pragma unroll
        for (int k = 0; k < N; ++k) { t[k] = 0; w[k] = 0.0; }
        for (int i = 0; i < R.m - 1; ++i) {
            R.get(i, g, h);
#pragma unroll
            for (int a = 0; a < N; ++a) {
                t[a] += g[a] * h;
#pragma unroll
                for (int b2 = 0; b2 <= a; ++b2) G[PK(a, b2)] += g[a] * g[b2];
            }
        }
        double tr = 0;
#pragma unroll
        for (int k = 0; k < N; ++k) tr += G[PK(k, k)];
#pragma unroll
        for (int k = 0; k < N; ++k) G[PK(k, k)] += 1e-12 * tr;
        if (chol<N>(G)) {
            chol_solve<N>(G, t);
#pragma unroll
            for (int k = 0; k < N; ++k) w[k] = t[k];
        }
    }
    double tmin = R_CAP, tmax = -1e300;
    for (int i = 0; i < R.m - 1; ++i) {
        R.get(i, g, h);
        double s = h;
#pragma unroll
        for (int k = 0; k < N; ++k) s -= g[k] * w[k];
        tmin = fmin(tmin, s / g[N]); tmax = fmax(tmax, s / g[N]);
    }
    double size = fmax(fabs(tmin), fmin(tmax, R_CAP) - tmin);
    if (!(size > 0.0)) size = 1.0;
    w[N] = tmin - size;
}

// one side of the bounding box of polytope p from its interior point `centre`: min (upper = 0) or max (upper = 1) of x_k
template <int N>
GCS_LP_HD int bound_lp(const Polys &S, int p, const double *centre, int k, int upper, double *lam, double *dlam, int lane, double &xk,
                       int *iters_out)
{
    Rows<N, false> R(S, p, -1);
    double w[N], c[N];
#pragma unroll
    for (int kk = 0; kk < N; ++kk) { w[kk] = centre[kk]; c[kk] = 0.0; }
    c[k] = upper ? -1.0 : 1.0;
    const int st = lp_ipm<N, false>(R, c, w, lam, dlam, lane, false, 0.0, iters_out);
    xk = w[k];
    return st;
}

} // namespace gcsadmm_lp
