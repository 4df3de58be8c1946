// gcs_math.h -- the numerics the three interior-point solvers on the device share: the wavefront program (vertex_program.inc), the
// workgroup program (vertex_wg.h) and the region-terminal solve (terminal_region.h).  Scalar and cone helpers, and the numerical
// decisions of DESIGN.md section 3 (stated independently in oracle/gcs_oracle.c, which the parity tests compare against).
// On the device the f64 reciprocal / reciprocal square root are the hardware estimates refined by Newton steps
// (an IEEE division costs ~100 dependent cycles on gfx950, a refined estimate ~25; tools/micro/rcp_accuracy.hip);
// on the host (debug emulation, tests/hostemu) they are the plain IEEE operations.
#pragma once
#include <math.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define GCS_HD __host__ __device__ __forceinline__
#else
#define GCS_HD inline
#endif

namespace gcs_math {

constexpr double REG_DELTA = 1e-7;    // Tikhonov term (REG_DELTA/2)|w|^2 on every centred unknown except t (oracle/gcs_oracle.c REG_DELTA)
constexpr double CHOL_SKIP = 1e-12;   // Cholesky pivot floor, relative to the pivot's own diagonal entry (oracle/gcs_oracle.c chol())

GCS_HD double rcp(double x)
{
#if defined(__HIP_DEVICE_COMPILE__)
    double r = __builtin_amdgcn_rcp(x);
    r = fma(fma(-x, r, 1.0), r, r);
    r = fma(fma(-x, r, 1.0), r, r);
    return r;
#else
    return 1.0 / x;
#endif
}

// one Newton step (relative error ~2e-15; the raw estimate has ~4.6e-8): slack reciprocals and step-length ratios
GCS_HD double rcp1(double x)
{
#if defined(__HIP_DEVICE_COMPILE__)
    const double r = __builtin_amdgcn_rcp(x);
    return fma(fma(-x, r, 1.0), r, r);
#else
    return 1.0 / x;
#endif
}

// the Cholesky pivots' reciprocal root: ~10 dependent instructions instead of ~35 for an IEEE sqrt and a reciprocal
GCS_HD double rsqrt_nr(double x)
{
#if defined(__HIP_DEVICE_COMPILE__)
    double r = __builtin_amdgcn_rsq(x);
    r = fma(0.5 * r, fma(-x * r, r, 1.0), r);
    r = fma(0.5 * r, fma(-x * r, r, 1.0), r);
    return r;
#else
    return 1.0 / sqrt(x);
#endif
}

// the refined reciprocal root and one Heron correction (an IEEE sqrt is ~140 dependent cycles)
GCS_HD double sqrt_nr(double x)
{
#if defined(__HIP_DEVICE_COMPILE__)
    if (!(x > 0.0)) return x < 0.0 ? __builtin_nan("") : x;   // 0 -> 0, NaN -> NaN
    const double r = rsqrt_nr(x);
    const double y = x * r;
    return fma(0.5 * r, fma(-y, y, x), y);
#else
    return sqrt(x);
#endif
}

// ---- second-order cone of dimension Q (first component = the epigraph variable) ----
template <int Q> GCS_HD double soc_det(const double *s)
{
    double nn = 0;
    for (int k = 1; k < Q; ++k) nn += s[k] * s[k];
    nn = sqrt_nr(nn);
    return (s[0] - nn) * (s[0] + nn);
}
template <int Q> GCS_HD bool soc_interior(const double *s)
{
    double nn = 0;
    for (int k = 1; k < Q; ++k) nn += s[k] * s[k];
    return s[0] > sqrt_nr(nn);
}
// largest step along ds that keeps s inside the cone (1e300: unbounded)
template <int Q> GCS_HD double soc_max_step(const double *s, const double *ds)
{
    double a = ds[0] * ds[0], b = s[0] * ds[0];
    const double c = soc_det<Q>(s);
    for (int k = 1; k < Q; ++k) { a -= ds[k] * ds[k]; b -= s[k] * ds[k]; }
    b *= 2;
    double al = 1e300;
    if (ds[0] < 0) al = fmin(al, -s[0] * rcp(ds[0]));
    if (fabs(a) < 1e-300) {
        if (b < 0) al = fmin(al, -c * rcp(b));
    } else {
        const double disc = b * b - 4 * a * c;
        if (disc >= 0) {
            const double sq = sqrt_nr(disc);
            const double qq = -0.5 * (b + (b >= 0 ? sq : -sq));
            const double r1 = qq * rcp(a), r2 = (qq != 0.0) ? c * rcp(qq) : 1e300;
            if (r1 > 0) al = fmin(al, r1);
            if (r2 > 0) al = fmin(al, r2);
        }
    }
    return al;
}
// Nesterov-Todd scaling of the cone from (s, z): wb (unit hyperbolic vector), eta; false on a boundary point
template <int Q> GCS_HD bool soc_scaling_wb(const double *s, const double *z, double *wb, double &eta)
{
    const double ss = soc_det<Q>(s), zz = soc_det<Q>(z);
    if (!(ss > 0.0) || !(zz > 0.0)) return false;
    const double is = rsqrt_nr(ss), iz = rsqrt_nr(zz);
    double dot = 0;
    for (int k = 0; k < Q; ++k) dot += (s[k] * is) * (z[k] * iz);
    const double ig2 = 0.5 * rsqrt_nr(0.5 * (1.0 + dot));   // 1 / (2 gamma)
    wb[0] = (s[0] * is + z[0] * iz) * ig2;
    for (int k = 1; k < Q; ++k) wb[k] = (s[k] * is - z[k] * iz) * ig2;
    eta = sqrt_nr((ss * is) * iz);   // (ss / zz)^(1/4)
    return true;
}

// ---- the rules of the interior-point iteration ----
// pivot d of a Cholesky / LDL' column whose diagonal entry was ref: a pivot that has cancelled below CHOL_SKIP * ref is round-off,
// not curvature, and is clamped to that floor
GCS_HD double pivot_floor(double d, double ref)
{
    if (!(d > CHOL_SKIP * ref)) d = ref > 0.0 ? CHOL_SKIP * ref : 1.0;
    return d;
}
// Mehrotra's centring parameter sigma from the ratio mu_aff / mu
GCS_HD double centring(double ratio)
{
    ratio = ratio < 0 ? 0 : (ratio > 1 ? 1 : ratio);
    return ratio * ratio * ratio;
}
// step length from the largest step amax that keeps every slack and dual inside its cone
GCS_HD double step_length(double amax) { return fmin(1.0, 0.99 * amax); }
// a step this short means the linear algebra has run out of precision
GCS_HD bool step_stalled(double al) { return al < 1e-3; }
// stop on the barrier parameter alone: at the tolerance, or within 1e3 of it after a stalled step; never on the first (re-centring)
// iteration of a warm solve
GCS_HD bool mu_converged(double mu, double tol, bool stalled, bool first_warm)
{
    return !first_warm && (mu <= tol || (stalled && mu <= 1e3 * tol));
}
// status of a solve whose cone pair has reached the boundary: accepted (0) when a cold solve is within 1e3 of the tolerance, failed
// (-4) otherwise
GCS_HD int boundary_status(double mu, double tol, bool warm) { return (mu <= 1e3 * tol && !warm) ? 0 : -4; }
// a non-finite step is precision exhausted too: at the last digits of a solve the Newton system can return NaN / Inf, which the ratio
// test does not see (fmin / fmax drop a NaN, so the step bound stays 1e300 and a full step of NaNs would be taken).  Such a step is
// not applied and counts as a stalled step, of length zero: the iterate stays as it is and mu_converged decides at the next stop test.
// probe: a sum of finite_probe(x) over entries x of the direction -- 0.0 when all are finite, NaN otherwise (a sum carries a NaN, a
// minimum or maximum does not)
GCS_HD double finite_probe(double x) { return x * 0.0; }
GCS_HD bool step_finite(double sigmu, double probe) { return sigmu - sigmu == 0.0 && probe == 0.0; }

} // namespace gcs_math
